"""GPU: the gain-match kernels (csrc/gain_match.hip, ``mod_extraction_amd.gain``) against their definition in numpy fp64
(tests/helpers/gain_match64.py).

Cases: N in {1, 5, CHUNK - 1, CHUNK, CHUNK + 3, 3 CHUNK + 1} x mode x B in {1, 3} x row stride {N, N + 1} x noise level
{1, 1e-4}.  y_hat, y, dz and the outputs each start 1, 2, 3 and 0 floats off a 16-byte boundary (torch's allocations are
aligned), so the leading array of every kernel and the arrays read beside it disagree about the head; with stride N + 1
every row starts somewhere else.  Row r of a case is y = K[r % 3] * (y_hat + 5 % noise) with K = (0.6, 0.01, 100) under
gain_range (0.05, 20): not clamped, clamped low, clamped high (B = 1 takes r = the case's index, so all three occur).

Gates, each from the arithmetic:
  sums    |got - exact| <= N 2^-53 sum |terms|: an fp64 sum of N exact products in any order (K19's gate); the helper's sums are
          exact (math.fsum of exact products).
  gain    2^-23 relative: one rounding to fp32 (2^-24) of a quotient of sums that are good to ~N 2^-53.
  z       2^-23 |z64| per element, z64 = g32 * y_hat in fp64: the kernel's z is its one rounding (2^-24) whenever the kernel's
          fp32 gain is the helper's; where the two gains are neighbours (the fp64 g within N 2^-53 of a rounding boundary)
          the gain test above still holds and this one may not -- none of the cases here is such a row, which is asserted.
  dy_hat  2^-23 (|g dz| + |s y / (a + eps)| + |2 s g y_hat / (a + eps)|) per element: one rounding (2^-24 of |dy_hat|, which
          is at most that sum) of an fp64 expression whose own error is ~1e-16 of the same magnitudes.  The helper is handed
          the kernel's gain, first sum and flag, as the backward kernel is.
  flags   equal.
The share of each gate that was used is printed (and recorded in profiles/r21/README.md).
"""
import numpy as np
import pytest
import torch

from tests.helpers import gain_match64 as h

pytestmark = pytest.mark.gpu
EPS = 1e-8
RANGE = (0.05, 20.0)
K = (0.6, 0.01, 100.0)
U = 2.0 ** -23


def sizes():
    from mod_extraction_amd.gain import CHUNK
    return [1, 5, CHUNK - 1, CHUNK, CHUNK + 3, 3 * CHUNK + 1]


def place(dev, arr, stride, offset):
    """``arr`` (B, N) on the device with rows ``stride`` floats apart, the first ``offset`` floats off an aligned allocation."""
    B, N = arr.shape
    flat = torch.full((offset + B * stride,), 7.0, device=dev, dtype=torch.float32)
    view = flat[offset:offset + B * stride].view(B, stride)[:, :N]
    view.copy_(torch.as_tensor(arr))
    assert view.data_ptr() % 16 == 4 * (offset % 4)
    return view


def gaps_untouched(view, stride, offset):
    """The floats between the rows of a ``place``d tensor (and before the first) still hold the fill value."""
    B, N = view.shape
    flat = view._base
    return bool((flat[:offset] == 7.0).all()) and bool((flat[offset:].view(B, stride)[:, N:] == 7.0).all())


def make_rows(B, N, level, case):
    rng = np.random.default_rng(1000 * N + 10 * B + case)
    p = (level * rng.standard_normal((B, N))).astype(np.float32)
    k = np.array([K[(r + (case if B == 1 else 0)) % 3] for r in range(B)])[:, None]
    q = (k * (p + 0.05 * level * rng.standard_normal((B, N)))).astype(np.float32)
    dz = rng.standard_normal((B, N)).astype(np.float32)
    return p, q, dz


def cases(N):
    return [(B, stride, level) for B in (1, 3) for stride in (N, N + 1) for level in (1.0, 1e-4)]


@pytest.mark.parametrize("mode", h.MODES)
@pytest.mark.parametrize("n_index", range(6))
def test_kernels_against_fp64(dev, mode, n_index):
    from mod_extraction_amd import gain as G
    N = sizes()[n_index]
    share = {"sums": 0.0, "gain": 0.0, "z": 0.0, "dy_hat": 0.0}
    seen_flags = set()
    for case, (B, stride, level) in enumerate(cases(N)):
        p, q, dz = make_rows(B, N, level, case)
        ref = h.rows64(p, q, mode, EPS, RANGE)
        tp, tq, td = place(dev, p, stride, 1), place(dev, q, stride, 2), place(dev, dz, stride, 3)
        out = place(dev, np.zeros_like(p), stride, 0)
        m = G.match_gain(tp, tq, mode, EPS, RANGE, out=out)
        assert m.z is out and m.gain.shape == (B,) and m.sums.shape == (B, 3) and m.flags.shape == (B,)
        sums, gain, flags, z = m.sums.cpu().numpy(), m.gain.cpu().numpy(), m.flags.cpu().numpy(), m.z.cpu().numpy()
        assert np.array_equal(flags, ref["flag"]), (B, stride, level)
        seen_flags.update(zip(flags.tolist(), (gain >= 1.0).tolist()))
        bound = N * 2.0 ** -53 * ref["abs_sums"]
        err = np.abs(sums - ref["sums"])
        assert (err <= bound).all(), (B, stride, level, err, bound)
        share["sums"] = max(share["sums"], float((err / bound).max()))
        err = np.abs(gain.astype(np.float64) - ref["g64"])
        assert (err <= U * np.abs(ref["g64"])).all(), (B, stride, level)
        share["gain"] = max(share["gain"], float((err / (U * np.abs(ref["g64"]))).max()))
        assert np.array_equal(gain, ref["g32"]), "a gain on a rounding boundary: choose another seed for this case"
        err = np.abs(z.astype(np.float64) - ref["z64"])
        assert (err <= U * np.abs(ref["z64"])).all(), (B, stride, level)
        share["z"] = max(share["z"], float((err / np.maximum(U * np.abs(ref["z64"]), 1e-300)).max()))
        assert gaps_untouched(out, stride, 0)
        # a second launch: the same bits
        m2 = G.match_gain(tp, tq, mode, EPS, RANGE)
        assert m2.z.is_contiguous() and all(torch.equal(u, v) for u, v in zip(m, m2))
        # backward, out of place into a strided out, then in place
        back = h.rows_backward64(dz, p, q, gain, sums[:, 0], flags, mode, EPS)
        dout = place(dev, np.zeros_like(p), stride, 0)
        d1 = G.match_gain_backward(td, tp, tq, m, mode, EPS, out=dout)
        assert d1 is dout and gaps_untouched(dout, stride, 0)
        got = d1.cpu().numpy().astype(np.float64)
        bound = U * back["scale"]
        err = np.abs(got - back["dy_hat"])
        assert (err <= bound).all(), (B, stride, level, float((err / np.maximum(bound, 1e-300)).max()))
        share["dy_hat"] = max(share["dy_hat"], float((err / np.maximum(bound, 1e-300)).max()))
        d2 = G.match_gain_backward(td, tp, tq, m, mode, EPS)
        assert torch.equal(d2, d1)
        keep = td.clone()
        d3 = G.match_gain_backward(td, tp, tq, m, mode, EPS, out=td)
        assert d3 is td and torch.equal(td, d1) and not torch.equal(td, keep)
        assert torch.equal(tp, torch.as_tensor(p).to(dev)) and torch.equal(tq, torch.as_tensor(q).to(dev))   # inputs are not written
    assert seen_flags >= {(0, False), (1, False), (1, True)}                  # not clamped, clamped low, clamped high
    print(f"N = {N} {mode}: share of each gate used " + ", ".join(f"{k} {v:.3f}" for k, v in share.items()))


def test_no_range_and_a_silent_row(dev):
    """Without ``gain_range`` nothing is clamped or flagged; a silent y_hat gives g = 0 under "ls" and sqrt((e + eps) / eps)
    under "rms", with finite outputs."""
    from mod_extraction_amd import gain as G
    N = G.CHUNK + 3
    p, q, dz = make_rows(3, N, 1.0, 0)
    p[1] = 0.0
    tp, tq, td = (torch.as_tensor(v).to(dev) for v in (p, q, dz))
    for mode in h.MODES:
        ref = h.rows64(p, q, mode, EPS, None)
        m = G.match_gain(tp, tq, mode, EPS, None)
        assert int(m.flags.sum()) == 0 and ref["flag"].sum() == 0
        assert np.array_equal(m.gain.cpu().numpy(), ref["g32"])
        assert float(m.gain[1]) == (0.0 if mode == "ls" else float(np.float32(np.sqrt((ref["sums"][1, 2] + EPS) / EPS))))
        assert bool((m.z[1] == 0).all()) and torch.isfinite(m.z).all()
        d = G.match_gain_backward(td, tp, tq, m, mode, EPS)
        back = h.rows_backward64(dz, p, q, m.gain.cpu().numpy(), m.sums[:, 0].cpu().numpy(), m.flags.cpu().numpy(), mode, EPS)
        assert torch.isfinite(d).all()
        assert (np.abs(d.cpu().numpy() - back["dy_hat"]) <= U * back["scale"]).all()


@pytest.mark.parametrize("mode", h.MODES)
def test_module_against_torch_autograd_in_fp64(dev, mode):
    """``MatchGain`` against torch autograd of the same expression in fp64 on the device, within the gates above.  The fp32
    rounding of g is applied as a constant offset (it has no derivative), the clamp as ``torch.clamp`` (zero slope outside)."""
    from mod_extraction_amd import gain as G
    B, N = 3, G.CHUNK + 3
    p, q, dz = make_rows(B, N, 1.0, 0)
    tp, tq, td = (torch.as_tensor(v).to(dev) for v in (p, q, dz))
    mod = G.MatchGain(mode, EPS, RANGE)
    x = tp.clone().requires_grad_(True)
    z = mod(x, tq)
    assert z.grad_fn is not None and not mod.last.gain.requires_grad
    (z * td).sum().backward()
    x64, y64, d64 = tp.double().requires_grad_(True), tq.double(), td.double()
    a, c, e = (x64 * x64).sum(1), (x64 * y64).sum(1), (y64 * y64).sum(1)
    g = c / (a + EPS) if mode == "ls" else torch.sqrt((e + EPS) / (a + EPS))
    g = torch.clamp(g, *RANGE)
    g = g + (g.detach().float().double() - g.detach())                          # the applied gain is the fp32 one
    z64 = g[:, None] * x64
    (z64 * d64).sum().backward()
    assert torch.equal(mod.last.gain, g.detach().float())
    assert mod.last.flags.tolist() == [0, 1, 1]
    assert bool(((z.detach().double() - z64.detach()).abs() <= U * z64.detach().abs()).all())
    k = torch.where(mod.last.flags.bool(), torch.zeros_like(a), (d64 * x64.detach()).sum(1) / (a.detach() + EPS))[:, None]
    scale = (g.detach()[:, None] * d64).abs() + (k * y64).abs() + (2.0 * k * g.detach()[:, None] * x64.detach()).abs()
    err = (x.grad.double() - x64.grad).abs()
    print(f"{mode}: share of the dy_hat gate used against autograd {float((err / (U * scale)).max()):.3f}")
    assert bool((err <= U * scale).all())


def test_exact_scaling(dev):
    """"ls", not clamped: y and 0.25 y give gain and z that are exactly 0.25 x (a power of two commutes with every rounding)."""
    from mod_extraction_amd import gain as G
    for N in (5, 3 * G.CHUNK + 1):
        p, q, _ = make_rows(3, N, 1.0, 0)
        q = (0.6 * p + 0.05 * np.random.default_rng(N).standard_normal(p.shape)).astype(np.float32)
        tp, tq = place(dev, p, N + 1, 1), place(dev, q, N + 1, 2)
        quarter = place(dev, 0.25 * q, N, 3)
        for rng in (None, RANGE):
            one, two = G.match_gain(tp, tq, "ls", EPS, rng), G.match_gain(tp, quarter, "ls", EPS, rng)
            assert int(one.flags.sum()) == 0 and int(two.flags.sum()) == 0
            assert torch.equal(two.gain, 0.25 * one.gain) and torch.equal(two.z, 0.25 * one.z)
            assert torch.equal(two.sums[:, 0], one.sums[:, 0]) and torch.equal(two.sums[:, 1], 0.25 * one.sums[:, 1])

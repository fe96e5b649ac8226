"""GPU: the FIR-match kernels (csrc/fir_match.hip, ``mod_extraction_amd.fir_match``, K21) against their definition in numpy
fp64 (tests/helpers/fir_match64.py), stage by stage, every stage on the kernel's own inputs.

Cases: N in {1, 5, 31, CHUNK - 1, CHUNK, CHUNK + 3, 3 CHUNK + 1} x K in {1, 2, 9, 32} x c in {0, (K - 1) // 2, K - 1} (N < K
included) x B in {1, 3} x row stride {N, N + 1} x level {1, 1e-4}.  y_hat, y and dz start 1, 2 and 3 floats off a 16-byte boundary; the
explicit outputs z and dy_hat start (case) % 4 and (case + 2) % 4 floats off one over the eight cases of a (N, K, c), so every
head size 0 .. 3 of the store path is taken on purpose, and with stride N + 1 every row starts somewhere else.  A row is a noise-driven comb,
y_hat = v[n] + 0.5 v[n - 7] with v white noise, and y = 0.6 y_hat[n - 1] + 0.3 y_hat[n] + 0.05 noise, both times the level.
ridge is 1e-6 where N >= CHUNK - 1 and 0.1 for the three short N, whose periodograms have deep nulls: with it the helper
reports cond(A) <= 100 on every row, which is asserted (``test_conditioning_of_the_cases``, on the CPU side of this file).

Gates, each from the arithmetic:
  sums    |got - exact| <= N 2^-53 sum |terms|: an fp64 sum of at most N exact products in any order; the helper's sums are exact
          (math.fsum).  Likewise gh, taken from the kernel's partials added in the kernel's order (chunk 0, 1, 2, ..).
  taps    2^-23 max |h|, h = the helper's solve on the KERNEL's sums: one fp32 rounding (2^-24) of a solution that two
          Cholesky solves in fp64 agree on to ~cond 2^-50.
  u, s    8 cond(A) N 2^-53 max |.|, the helper's bwd_solve on the kernel's gh, R and taps.
  z       2^-23 sum_k |taps[k] x[n + c - k]| per element, the helper's apply on the kernel's taps: one rounding of an fp64 sum.
  dy_hat  2^-23 (the sum of the 4K - 1 terms' magnitudes) per element, the helper's bwd_apply on the kernel's taps, u, s.
  flags   equal to the helper's (on the kernel's sums).
The share of each gate that was used is printed; MODEX_FIR_REPORT=<file> appends it as JSON lines (on record in
profiles/r22/measured_errors_gpu_tests.json; the table is in profiles/r22/fir_match.md).
"""
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import fir_match64 as h

EPS = 1e-8
MAX_GAIN = 20.0
U = 2.0 ** -23
CHUNK = 2048
SIZES = [1, 5, 31, CHUNK - 1, CHUNK, CHUNK + 3, 3 * CHUNK + 1]
TAPS = [1, 2, 9, 32]
_REPORT = os.environ.get("MODEX_FIR_REPORT")


def ridge_of(N):
    return 1e-6 if N >= CHUNK - 1 else 0.1


def centres(K):
    return sorted({0, (K - 1) // 2, K - 1})


def cases(N):
    return [(B, stride, level) for B in (1, 3) for stride in (N, N + 1) for level in (1.0, 1e-4)]


def make_rows(B, N, level, case):
    rng = np.random.default_rng(1000 * N + 10 * B + case)
    v = rng.standard_normal((B, N + 8))
    p = (level * (v[:, 8:] + 0.5 * v[:, 1:N + 1])).astype(np.float32)
    q = 0.3 * p.astype(np.float64) + 0.05 * level * rng.standard_normal((B, N))
    q[:, 1:] += 0.6 * p[:, :-1]
    return p, q.astype(np.float32), rng.standard_normal((B, N)).astype(np.float32)


def report(name, share):
    print(f"{name}: share of each gate used " + ", ".join(f"{k} {v:.3f}" for k, v in share.items()))
    if _REPORT:
        with open(_REPORT, "a") as f:
            f.write(json.dumps({"test": name, "share_of_gate": share}) + "\n")


def test_conditioning_of_the_cases():
    """CPU: cond(A) <= 100 on every row of every case (the u / s gate is stated in it)."""
    from mod_extraction_amd.fir_match import CHUNK as chunk
    assert chunk == CHUNK
    worst = 0.0
    for N in SIZES:
        for case, (B, stride, level) in enumerate(cases(N)):
            p, q, _ = make_rows(B, N, level, case)
            for row in p.astype(np.float64):
                R = np.array([np.dot(row[:max(N - d, 0)], row[d:]) for d in range(max(TAPS))])   # plain sums do for cond
                for K in TAPS:
                    worst = max(worst, float(np.linalg.cond(h.system(R[:K], ridge_of(N), EPS))))
    print(f"worst cond(A) over the cases: {worst:.2f}")
    assert worst <= 100.0


def place(dev, arr, stride, offset):
    """``arr`` (B, N) on the device with rows ``stride`` floats apart, the first ``offset`` floats off an aligned allocation."""
    B, N = arr.shape
    flat = torch.full((offset + B * stride,), 7.0, device=dev, dtype=torch.float32)
    view = flat[offset:offset + B * stride].view(B, stride)[:, :N]
    view.copy_(torch.as_tensor(arr))
    assert view.data_ptr() % 16 == 4 * (offset % 4)
    return view


def gaps_untouched(view, stride, offset):
    B, N = view.shape
    flat = view._base
    return bool((flat[:offset] == 7.0).all()) and bool((flat[offset:].view(B, stride)[:, N:] == 7.0).all())


def frac(err, bound):
    return float((err / np.maximum(bound, 1e-300)).max())


@pytest.mark.gpu
@pytest.mark.parametrize("K", TAPS)
@pytest.mark.parametrize("n_index", range(len(SIZES)))
def test_kernels_against_fp64(dev, n_index, K):
    from mod_extraction_amd import fir_match as F
    N, ridge = SIZES[n_index], ridge_of(SIZES[n_index])
    share = {"sums": 0.0, "taps": 0.0, "z": 0.0, "gh": 0.0, "u": 0.0, "s": 0.0, "dy_hat": 0.0}
    for c in centres(K):
        for case, (B, stride, level) in enumerate(cases(N)):
            tag = (N, K, c, B, stride, level)
            p, q, dz = make_rows(B, N, level, case)
            tp, tq, td = place(dev, p, stride, 1), place(dev, q, stride, 2), place(dev, dz, stride, 3)
            out = place(dev, np.zeros_like(p), stride, case % 4)
            m = F.match_fir(tp, tq, K, c, ridge, EPS, MAX_GAIN, out=out)
            assert m.z is out and m.taps.shape == (B, K) and m.sums.shape == (B, 2 * K + 1) and m.flags.shape == (B,)
            sums, taps, flags, z = (t.cpu().numpy() for t in (m.sums, m.taps, m.flags, m.z))
            assert gaps_untouched(out, stride, case % 4)
            m2 = F.match_fir(tp, tq, K, c, ridge, EPS, MAX_GAIN)               # a second launch: the same bits
            assert m2.z.is_contiguous() and all(torch.equal(a, b) for a, b in zip(m, m2))
            dout = place(dev, np.zeros_like(p), stride, (case + 2) % 4)
            d1, gh_parts, u, s = F._backward_parts(td, tp, tq, m, ridge, EPS, c, out=dout)
            assert d1 is dout and gaps_untouched(dout, stride, (case + 2) % 4)
            assert torch.equal(F.match_fir_backward(td, tp, tq, m, ridge, EPS, c), d1)
            got = d1.cpu().numpy().astype(np.float64)
            gh_parts, u, s = (t.cpu().numpy() for t in (gh_parts, u, s))
            assert gh_parts.shape == (B, F.n_chunks(N), K) and u.shape == (B, K) and s.shape == (B, 2 * K - 1)
            for r in range(B):
                ref = h.sums(p[r], q[r], K, c)
                bound = N * 2.0 ** -53 * ref["abs_sums"]
                err = np.abs(sums[r] - ref["sums"])
                assert (err <= bound).all(), (tag, r, err, bound)
                share["sums"] = max(share["sums"], frac(err, bound))
                sol = h.solve(sums[r], K, c, ridge, EPS, MAX_GAIN)
                assert sol["cond"] <= 100.0 and flags[r] == sol["flag"] == 0, (tag, r, sol["cond"], flags[r])
                bound = U * np.abs(sol["h64"]).max()
                err = np.abs(taps[r].astype(np.float64) - sol["h64"])
                assert (err <= bound).all(), (tag, r)
                share["taps"] = max(share["taps"], frac(err, bound))
                ap = h.apply(p[r], taps[r], c)
                err = np.abs(z[r].astype(np.float64) - ap["z64"])
                assert (err <= U * ap["scale"]).all(), (tag, r, frac(err, U * ap["scale"]))
                share["z"] = max(share["z"], frac(err, U * ap["scale"]))
                gh = np.zeros(K)
                for chunk in gh_parts[r]:                                      # the kernel's order
                    gh = gh + chunk
                bs = h.bwd_sums(dz[r], p[r], K, c)
                bound = N * 2.0 ** -53 * bs["abs_gh"]
                err = np.abs(gh - bs["gh"])
                assert (err <= bound).all(), (tag, r, err, bound)
                share["gh"] = max(share["gh"], frac(err, bound))
                want = h.bwd_solve(gh, sums[r, :K], taps[r], 0, ridge, EPS)
                for name, mine in (("u", u[r]), ("s", s[r])):
                    bound = 8.0 * sol["cond"] * N * 2.0 ** -53 * np.abs(want[name]).max()
                    err = np.abs(mine - want[name])
                    assert (err <= bound).all(), (tag, r, name, frac(err, bound))
                    share[name] = max(share[name], frac(err, bound))
                ba = h.bwd_apply(dz[r], q[r], p[r], taps[r], u[r], s[r], c)
                err = np.abs(got[r] - ba["dy_hat"])
                assert (err <= U * ba["scale"]).all(), (tag, r, frac(err, U * ba["scale"]))
                share["dy_hat"] = max(share["dy_hat"], frac(err, U * ba["scale"]))
            for t, a in ((tp, p), (tq, q), (td, dz)):                          # inputs are not written
                assert torch.equal(t, torch.as_tensor(a).to(dev))
    report(f"kernels N = {N} K = {K}", share)


@pytest.mark.gpu
def test_hand_made_rows_trip_each_guard(dev):
    """Rows: 0 ordinary; 1 silent y_hat with a tiny eps: h = 0, not flagged; 2 taps beyond max_gain: flag 2; 3 y_hat with an
    inf: the first pivot is not finite, flag 1; 4 y = -y of row 0: negative taps, not flagged.  A flagged row gives z = y_hat
    and dy_hat = dz bit for bit (zero taps read nothing, so the inf stays one sample and makes no NaN)."""
    from mod_extraction_amd import fir_match as F
    N, K, c, eps = CHUNK + 3, 9, 4, 1e-300
    p, q, dz = make_rows(5, N, 1.0, 0)
    p[1] = 0.0
    q[2] = 1000.0 * q[2]
    p[3, 5] = np.inf
    p[4], q[4] = p[0], -q[0]
    tp, tq, td = (torch.as_tensor(v).to(dev) for v in (p, q, dz))
    m = F.match_fir(tp, tq, K, c, 1e-6, eps, MAX_GAIN)
    ref = h.rows64(p, q, K, c, 1e-6, eps, MAX_GAIN)
    assert m.flags.tolist() == ref["flag"].tolist() == [0, 0, 2, 1, 0]
    identity = [0.0] * c + [1.0] + [0.0] * (K - 1 - c)
    assert m.taps[2].tolist() == identity and m.taps[3].tolist() == identity
    assert not m.taps[1].any() and not m.z[1].any() and torch.equal(m.taps[4], -m.taps[0]) and torch.equal(m.z[4], -m.z[0])
    assert torch.equal(m.z[2], tp[2]) and torch.equal(m.z[3], tp[3]) and not torch.isnan(m.z).any()
    d, _, u_all, s_all = F._backward_parts(td, tp, tq, m, 1e-6, eps, c)
    parts = {"u": u_all, "s": s_all}
    assert torch.equal(d[2], td[2]) and torch.equal(d[3], td[3]) and not torch.isnan(d).any()
    for r in (2, 3):
        assert not parts["u"][r].any() and not parts["s"][r].any()
    assert torch.equal(d[1], torch.zeros_like(d[1]))                           # h = 0 and u = 0 / eps-regular: nothing flows
    for r in (0, 4):
        ba = h.bwd_apply(dz[r], q[r], p[r], m.taps[r].cpu().numpy(), parts["u"][r].cpu().numpy(), parts["s"][r].cpu().numpy(), c)
        assert (np.abs(d[r].cpu().numpy() - ba["dy_hat"]) <= U * ba["scale"]).all()


@pytest.mark.gpu
def test_exact_scaling(dev):
    """y and 0.25 y give exactly 0.25 x the taps and z: b is a sum of exact products, the two triangular solves are linear in
    their right-hand side, and a power of two commutes with every rounding."""
    from mod_extraction_amd import fir_match as F
    for N, K in ((5, 2), (3 * CHUNK + 1, 9), (CHUNK, 32)):
        p, q, _ = make_rows(3, N, 1.0, 0)
        tp, tq = place(dev, p, N + 1, 1), place(dev, q, N + 1, 2)
        quarter = place(dev, 0.25 * q, N, 3)
        one, two = F.match_fir(tp, tq, K, None, ridge_of(N)), F.match_fir(tp, quarter, K, None, ridge_of(N))
        assert int(one.flags.sum()) == 0 and int(two.flags.sum()) == 0
        assert torch.equal(two.taps, 0.25 * one.taps) and torch.equal(two.z, 0.25 * one.z)
        assert torch.equal(two.sums[:, :K], one.sums[:, :K]) and torch.equal(two.sums[:, K:2 * K], 0.25 * one.sums[:, K:2 * K])


@pytest.mark.gpu
def test_one_tap_is_the_ls_gain(dev):
    """K = 1, ridge = 0 against K20's kernels: the same gain to one rounding (Cholesky divides twice by sqrt(a + eps), K20 once
    by a + eps: 2^-23 relative covers both roundings to fp32), the same sums to their gate."""
    from mod_extraction_amd import fir_match as F
    from mod_extraction_amd.gain import match_gain
    p, q, _ = make_rows(3, CHUNK + 3, 1.0, 1)
    tp, tq = torch.as_tensor(p).to(dev), torch.as_tensor(q).to(dev)
    m, g = F.match_fir(tp, tq, 1, 0, 0.0, EPS), match_gain(tp, tq, "ls", EPS)
    assert bool(((m.taps[:, 0] - g.gain).abs() <= U * g.gain.abs()).all())
    ref = h.rows64(p, q, 1, 0, 0.0, EPS)
    for got in (m.sums.cpu().numpy(), g.sums.cpu().numpy()):
        assert (np.abs(got - ref["sums"]) <= p.shape[1] * 2.0 ** -53 * ref["abs_sums"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("K, c", [(1, 0), (9, 4), (9, 0), (32, 31)])
def test_module_against_the_fp64_composition(dev, K, c):
    """``MatchFir`` under autograd against the helper's composition (its own sums, solve and fp32 taps): d loss / d y_hat
    norm-wise within 3e-6, the project's chain gate; z within its per-element gate where the two sets of taps are the same
    fp32 values, which is asserted."""
    from mod_extraction_amd import fir_match as F
    from tests.test_gpu_flanger_grad import normwise
    B, N = 3, CHUNK + 3
    p, q, dz = make_rows(B, N, 1.0, 2)
    tp, tq, td = (torch.as_tensor(v).to(dev) for v in (p, q, dz))
    mod = F.MatchFir(K, c, 1e-6, EPS, MAX_GAIN)
    x = tp.clone().requires_grad_(True)
    z = mod(x, tq)
    assert z.grad_fn is not None and not mod.last.taps.requires_grad and tq.grad is None
    (z * td).sum().backward()
    fwd = h.rows64(p, q, K, c, 1e-6, EPS, MAX_GAIN)
    back = h.rows_backward64(dz, p, q, fwd, c, 1e-6, EPS)
    assert mod.last.flags.tolist() == [0, 0, 0] and np.array_equal(mod.last.taps.cpu().numpy(), fwd["taps"])
    assert (np.abs(z.detach().cpu().numpy() - fwd["z64"]) <= U * fwd["scale"]).all()
    err = normwise(x.grad.cpu().numpy(), back["dy_hat"], slice(None))
    report(f"module K = {K} c = {c}", {"chain_3e-6": err / 3e-6})
    assert err < 3e-6

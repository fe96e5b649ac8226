"""GPU: the shaper-match kernels (csrc/shaper_match.hip, ``mod_extraction_amd.shaper``, K27) against their definition in numpy
fp64 (tests/helpers/shaper_match64.py), stage by stage, every stage on the kernel's own inputs.

Cases: N in {1, 5, 31, CHUNK - 1, CHUNK, CHUNK + 3, 3 CHUNK + 1} x order in {1, 3, 5, 7} x even x B in {1, 3} x row stride
{N, N + 1} x amplitude {1, 1e-4}.  y_hat, y and dz start 1, 2 and 3 floats off a 16-byte boundary; the explicit outputs z and dy_hat
start (case) % 4 and (case + 2) % 4 floats off one over the eight cases of a (N, order, even), so every head size 0 .. 3 of the store
path is taken, and with stride N + 1 every row starts somewhere else.  A row is a noise-driven comb x[n] + 0.7 x[n - 37] at the given
peak, and y a soft clip of it with an even part, 0.25 pk tanh(2 x / pk) + 0.05 x^2 / pk.  Every case runs with the default ridge
1e-9.  Rows shorter than the number of coefficients (N = 1, 5 against K up to 7) have a singular Gram matrix, which only the ridge
keeps positive: its small pivots are then 1e-9 .. 4e-8 of the largest, seven orders above their rounding error, and cond(A) reaches
5e10 -- the coefficient and u gates are stated in cond(A), so they widen with it.  ``test_the_cases_are_unflagged`` (on the CPU side
of this file) asserts that the helper flags no row of any case, that every pivot stays above 1e-10 of the largest, and reports the
worst cond(A).

Gates, each from the arithmetic (u = 2^-53):
  sums    |got - ref| <= (N + 2 P) u sum |terms|: an fp64 sum of N terms in any order, each term a power of t formed by at most
          2 P - 1 roundings (and one product more for b); ref is the helper on the kernel's own r.
  coeffs  64 cond(A) u max |c| + 2^-23 max |c|, c = the helper's solve on the KERNEL's sums: a component passes through at most
          K^2 + 2 K <= 63 roundings of the factorisation and the two substitutions, each amplified by at most cond(A); then one
          fp32 rounding (2^-24, doubled).
  z       2^-23 |ref| per element, ref = the helper's Horner on the kernel's coeffs and r: the one rounding to fp32 (2^-24) and
          as much again for the fp64 evaluation.
  g       (N + P) u sum |terms|, as the sums.
  u       64 cond(A) u max |u| + |A^-1| n_chunks u |sum_chunks |partials||: the helper's solve on the kernel's partials added
          chunk by chunk, which the kernel adds in another order.
  dy_hat  2^-23 |ref| per element, ref = the helper's bwd_apply on the kernel's coeffs, r and u: two fp32 roundings of the fp64
          value.  The sum of 5 K products may cancel, but the helper performs the kernel's operations in the kernel's order and the
          library is built without contraction, so no allowance for the fp64 evaluation is made.
  flags   equal to the helper's (on the kernel's sums).
The share of each gate that was used is printed; MODEX_SHAPER_REPORT=<file> appends it as JSON lines.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import shaper_match64 as h

U53, U23 = 2.0 ** -53, 2.0 ** -23
CHUNK = h.CHUNK
SIZES = [1, 5, 31, CHUNK - 1, CHUNK, CHUNK + 3, 3 * CHUNK + 1]
CONFIGS = [(P, even) for P in (1, 3, 5, 7) for even in (False, True)]
MAX_GAIN = 20.0
_REPORT = os.environ.get("MODEX_SHAPER_REPORT")


def ridge_of(N, order, even):
    return 1e-9


def cases(N):
    return [(B, stride, amp) for B in (1, 3) for stride in (N, N + 1) for amp in (1.0, 1e-4)]


def make_rows(B, N, amp, case):
    rng = np.random.default_rng(1000 * N + 10 * B + case)
    p = np.stack([h.comb(N, 77 * N + 13 * B + case + 101 * r, amp) for r in range(B)])
    x = p.astype(np.float64)
    q = 0.25 * amp * np.tanh(2.0 * x / amp) + 0.05 * x * x / amp
    return p, q.astype(np.float32), rng.standard_normal((B, N)).astype(np.float32)


def report(name, share):
    print(f"{name}: share of each gate used " + ", ".join(f"{k} {v:.3g}" for k, v in share.items()))
    if _REPORT:
        with open(_REPORT, "a") as f:
            f.write(json.dumps({"test": name, "share_of_gate": share}) + "\n")


def test_the_cases_are_unflagged():
    """CPU: the helper flags no row of any case (the poison test's first two rows included) and no pivot comes near 0."""
    worst, low = 0.0, 1.0
    for N in SIZES:
        for order, even in CONFIGS:
            rows = [make_rows(B, N, amp, case)[:2] for case, (B, stride, amp) in enumerate(cases(N))]
            if N in (5, CHUNK + 3):
                rows.append(tuple(a[:2] for a in make_rows(3, N, 1.0, 3)[:2]))
            for p, q in rows:
                for x, y in zip(p, q):
                    f = h.forward(x, y, order, even, ridge_of(N, order, even), MAX_GAIN)
                    assert f["flag"] == 0, (N, order, even, f["pivots"], f["c"])
                    worst = max(worst, float(np.linalg.cond(h.gram(f["sums"], order, even, ridge_of(N, order, even))[0])))
                    low = min(low, min(f["pivots"]) / max(f["pivots"]))
    print(f"worst cond(A) over the cases: {worst:.3g}; smallest pivot / largest: {low:.3g}")
    assert low > 1e-10


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
    return float(np.max(np.asarray(err) / np.maximum(np.asarray(bound), 1e-300)))


@pytest.mark.gpu
@pytest.mark.parametrize("order,even", CONFIGS)
@pytest.mark.parametrize("n_index", range(len(SIZES)))
def test_kernels_against_fp64(dev, n_index, order, even):
    from mod_extraction_amd import shaper as S
    N = SIZES[n_index]
    ridge, K, ns = ridge_of(N, order, even), len(h.powers(order, even)), h.n_sums(order, even)
    share = {"sums": 0.0, "coeffs": 0.0, "z": 0.0, "g": 0.0, "u": 0.0, "dy_hat": 0.0}
    for case, (B, stride, amp) in enumerate(cases(N)):
        tag = (N, order, even, B, stride, amp)
        p, q, dz = make_rows(B, N, amp, case)
        tp, tq, td = place(dev, p, stride, 1), place(dev, q, stride, 2), place(dev, dz, stride, 3)
        out = place(dev, np.zeros_like(p), stride, case % 4)
        m, parts = S._forward_parts(tp, tq, order, even, ridge, MAX_GAIN, out=out)
        assert m.z is out and m.coeffs.shape == (B, K) and m.scale.shape == (B,) and m.sums.shape == (B, ns) and m.flags.shape == (B,)
        assert parts.shape == (B, S.n_chunks(N), ns) and gaps_untouched(out, stride, case % 4)
        m2 = S.match_shaper(tp, tq, order, even, ridge, MAX_GAIN)            # a second launch: the same bits
        assert m2.z.is_contiguous() and all(torch.equal(a, b) for a, b in zip(m, m2))
        dout = place(dev, np.zeros_like(p), stride, (case + 2) % 4)
        d1, g_parts, u = S._backward_parts(td, tp, tq, m, even, ridge, out=dout)
        assert d1 is dout and gaps_untouched(dout, stride, (case + 2) % 4)
        assert torch.equal(S.match_shaper_backward(td, tp, tq, m, even, ridge), d1)
        td2 = place(dev, dz, stride, 3)
        assert S.match_shaper_backward(td2, tp, tq, m, even, ridge, out=td2) is td2 and torch.equal(td2, d1)   # in place
        assert gaps_untouched(td2, stride, 3)
        sums, coeffs, scale, flags, z, got, g_parts, u, parts = (
            t.cpu().numpy() for t in (m.sums, m.coeffs, m.scale, m.flags, m.z, d1, g_parts, u, parts))
        assert g_parts.shape == (B, S.n_chunks(N), K) and u.shape == (B, K)
        for r in range(B):
            rr = float(scale[r])
            S2, r_ref, bad = h.scale(p[r])
            assert not bad and abs(rr - r_ref) <= 2.0 ** -23 * r_ref, (tag, r, rr, r_ref)
            ref, mag = h.sums(p[r], q[r], order, even, r=rr)
            bound = (N + 2 * order) * U53 * mag
            err = np.abs(sums[r] - ref)
            assert (err <= bound).all(), (tag, r, err, bound)
            share["sums"] = max(share["sums"], frac(err, bound))
            c64, r_sol, flag, piv = h.solve(sums[r], N, order, even, ridge, MAX_GAIN, round32=False)
            assert flags[r] == flag == 0 and r_sol == rr, (tag, r, flags[r], flag, piv)
            A, _ = h.gram(sums[r], order, even, ridge)
            cond = float(np.linalg.cond(A))
            bound = (64 * cond * U53 + U23) * np.abs(c64).max()
            err = np.abs(coeffs[r].astype(np.float64) - c64)
            assert (err <= bound).all(), (tag, r, cond, err, bound)
            share["coeffs"] = max(share["coeffs"], frac(err, bound))
            c32 = coeffs[r].astype(np.float64)
            zref = h.apply(p[r], c32, rr, order, even)
            err, bound = np.abs(z[r] - zref), U23 * np.abs(zref) + 2.0 ** -149
            assert (err <= bound).all(), (tag, r, frac(err, bound))
            share["z"] = max(share["z"], frac(err, bound))
            gref, gmag = h.bwd_sums(dz[r], p[r], rr, order, even)
            gk = g_parts[r].sum(0)
            err, bound = np.abs(gk - gref), (N + order) * U53 * gmag
            assert (err <= bound).all(), (tag, r, err, bound)
            share["g"] = max(share["g"], frac(err, bound))
            uref = h.bwd_solve(gk, sums[r], order, even, ridge)
            bound = 64 * cond * U53 * np.abs(uref).max() + (np.linalg.norm(np.linalg.inv(A), 2) * g_parts.shape[1] * U53
                                                           * np.linalg.norm(np.abs(g_parts[r]).sum(0)))
            err = np.abs(u[r] - uref)
            assert (err <= bound).all(), (tag, r, cond, err, bound)
            share["u"] = max(share["u"], frac(err, bound))
            dref, dmag = h.bwd_apply(dz[r], p[r], q[r], c32, rr, u[r], order, even, ridge)
            err, bound = np.abs(got[r] - dref), U23 * np.abs(dref) + 2.0 ** -149
            assert (err <= bound).all(), (tag, r, frac(err, bound))
            share["dy_hat"] = max(share["dy_hat"], frac(err, bound))
    report(f"shaper N={N} order={order} even={even}", share)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("order,even", [(5, False), (4, True)])
def test_flagged_rows(dev, order, even):
    """Five rows of 4096 samples: a plain one; y = 400 x (sum |c| over max_gain: flag 2); a silent one and one with a NaN in it
    (S2: flag 1); and a constant 1/2, where r = 1/2, t = 1, every moment is 4096 and sqrt(4096) = 64, so the factorisation is
    exact in the kernel and in the helper alike and, without a ridge, the second pivot is exactly 0 (flag 1).
    The pivots of the other rows are far from 0.  Flagged rows copy y_hat and dz bit for bit."""
    from mod_extraction_amd import shaper as S
    N, ridge = 4096, 0.0
    p, q, dz = make_rows(5, N, 1.0, 0)
    q[1] = 400.0 * p[1]
    p[2] = 0.0
    p[3, 1000] = np.nan
    p[4] = 0.5
    tp, tq, td = place(dev, p, N + 1, 1), place(dev, q, N + 1, 2), place(dev, dz, N + 1, 3)
    m = S.match_shaper(tp, tq, order, even, ridge, MAX_GAIN)
    d = S.match_shaper_backward(td, tp, tq, m, even, ridge)
    sums, flags, coeffs = m.sums.cpu().numpy(), m.flags.cpu().numpy(), m.coeffs.cpu().numpy()
    K = len(h.powers(order, even))
    want = [0, 2, 1, 1, 1]
    for r in range(5):
        c, _, flag, piv = h.solve(sums[r], N, order, even, ridge, MAX_GAIN)
        assert flags[r] == flag == want[r], (r, flags[r], flag, piv)
        if r < 2:
            assert min(piv) > 1e-6 * max(piv)                               # well away from the threshold
        if want[r]:
            assert coeffs[r].tolist() == [1.0] + [0.0] * (K - 1)
            assert torch.equal(bits(m.z[r]), bits(tp[r])) and torch.equal(bits(d[r]), bits(td[r]))
    assert m.scale.cpu().tolist()[2:] == [1.0, 1.0, 0.5]
    assert h.solve(sums[4], N, order, even, ridge, MAX_GAIN)[3][:2] == [4096.0, 0.0]
    td2 = place(dev, dz, N + 1, 3)
    S.match_shaper_backward(td2, tp, tq, m, even, ridge, out=td2)
    assert torch.equal(bits(td2), bits(d))
    assert not torch.equal(d[0], td[0]) and not torch.equal(m.z[0], tp[0])


@pytest.mark.gpu
@pytest.mark.parametrize("N", [31, CHUNK + 3])
def test_order_one_is_the_ls_gain(dev, N):
    """c_1 against ``match_gain("ls")`` (its eps far below the energy, the ridge 0) within 2^-22: both are one fp32 rounding
    of fp64 quotients that agree to a few 2^-53.  z within 5 2^-24: the two gains' roundings, the two products' roundings and
    the fp64 detour through x / r."""
    from mod_extraction_amd import gain, shaper as S
    p, q, _ = make_rows(3, N, 1.0, 1)
    tp, tq = place(dev, p, N + 1, 1), place(dev, q, N + 1, 2)
    m = S.match_shaper(tp, tq, 1, False, 0.0, MAX_GAIN)
    g = gain.match_gain(tp, tq, "ls", 1e-30, None)
    c, gg = m.coeffs[:, 0].double(), g.gain.double()
    assert m.flags.tolist() == [0, 0, 0] and bool(((c - gg).abs() <= 2.0 ** -22 * gg.abs()).all())
    assert bool(((m.z.double() - g.z.double()).abs() <= 5 * 2.0 ** -24 * g.z.double().abs()).all())


@pytest.mark.gpu
@pytest.mark.parametrize("order,even", [(5, False), (7, True)])
def test_scaling_invariances_are_bit_exact(dev, order, even):
    from mod_extraction_amd import shaper as S
    N = CHUNK + 3
    p, q, dz = make_rows(3, N, 1.0, 2)
    tp, tq, td = place(dev, p, N + 1, 1), place(dev, q, N + 1, 2), place(dev, dz, N, 3)
    a = S.match_shaper(tp, tq, order, even)
    b = S.match_shaper(tp, place(dev, 0.25 * q, N + 1, 2), order, even)
    assert a.flags.tolist() == b.flags.tolist() == [0, 0, 0]
    assert torch.equal(b.coeffs, 0.25 * a.coeffs) and torch.equal(b.z, 0.25 * a.z) and torch.equal(b.scale, a.scale)
    tp4, tq4 = place(dev, 0.25 * p, N + 1, 1), place(dev, 0.25 * q, N + 1, 2)
    c = S.match_shaper(tp4, tq4, order, even)
    assert torch.equal(c.coeffs, a.coeffs) and torch.equal(c.z, 0.25 * a.z) and torch.equal(c.scale, 0.25 * a.scale)
    assert torch.equal(c.sums[:, 1:-1], a.sums[:, 1:-1]) and c.flags.tolist() == [0, 0, 0]
    # the backward: the curve's slope does not change with the common level
    da = S.match_shaper_backward(td, tp, tq, a, even, 1e-9)
    dc = S.match_shaper_backward(td, tp4, tq4, c, even, 1e-9)
    assert torch.equal(da, dc)


@pytest.mark.gpu
@pytest.mark.parametrize("order,even", [(1, False), (5, False), (7, True)])
@pytest.mark.parametrize("N", [5, CHUNK + 3])
def test_uninitialised_memory_changes_no_bit(dev, N, order, even):
    """The 0 / 0.5 / NaN fills of tests/helpers/poison_alloc.py: z, the coefficients, the scale, the sums, the flags, both
    workspaces, u and dy_hat come from ``torch.empty``; a flagged row is among the rows."""
    from mod_extraction_amd import shaper as S
    from tests.test_gpu_uninit_independence import _dv, run_patterns
    p, q, dz = make_rows(3, N, 1.0, 3)
    q[2] = 400.0 * p[2]
    y_hat, y, d = _dv(dev, p), _dv(dev, q), _dv(dev, dz)
    ridge = ridge_of(N, order, even)

    def case():
        m, parts = S._forward_parts(y_hat, y, order, even, ridge, MAX_GAIN)
        dy, g_parts, u = S._backward_parts(d, y_hat, y, m, even, ridge)
        return {"z": m.z, "coeffs": m.coeffs, "scale": m.scale, "sums": m.sums, "flags": m.flags, "partials": parts,
                "dy_hat": dy, "g_partials": g_parts, "u": u}

    run_patterns(case, {"shaper:_forward_parts", "shaper:_backward_parts"})
    assert S.match_shaper(y_hat, y, order, even, ridge, MAX_GAIN).flags.tolist() == [0, 0, 2]

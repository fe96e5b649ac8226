"""CPU: the numpy fp64 restatement of the lag and polarity estimate (tests/helpers/pair_align64.py, K19) on the table the GPU
test compares the kernels on: (N, L) in {(257, 8), (4096, 64), (4099, 129)} x {white, pink} dry rows x a wet that lags the
dry by lag in {-L, -3, 0, 1, L} x polarity +1 / -1, the wet a comb ``pol (x + 0.5 x[n - d(n)])`` with a tap swinging over
5 .. 35 samples, cut from a longer render so that no zeros enter.

The table has to be recovered exactly, and the peak |c| has to stand at least MIN_GAP = 0.03 above the runner-up on these seeds:
a condition on the TABLE (it keeps the GPU comparison from hinging on a near-tie; differences of fp64 summation order are
around 1e-16), not a measurement of any kernel.  The gap is about 0.75 on the white rows and 0.047 .. 0.09 on the pink ones,
whose neighbouring lags correlate at 0.9 (smallest: 0.0471 at N = 257, 0.0744 at the two long sizes).
"""
import numpy as np
import pytest

from tests.helpers import pair_align64 as h

MIN_GAP = 0.03


@pytest.mark.parametrize("N,L", h.SIZES)
def test_table_is_recovered_exactly_with_a_gap(N, L):
    worst = np.inf
    for (n, l, kind, lag, pol) in h.table():
        if (n, l) != (N, L):
            continue
        dry, wet = h.make_pair(N, L, kind, lag, pol)
        assert dry.dtype == wet.dtype == np.float32 and dry.shape == wet.shape == (N,)
        assert np.all(wet != 0.0)                                             # cut from a longer render: no zero fill
        e = h.estimate64(dry, wet, L)
        print(f"N {N} L {L} {kind:5s} lag {lag:4d} pol {pol:+d}: found {e['lag']:4d} corr {e['corr']:+.4f} frac {e['frac']:+.4f} "
              f"gap {e['gap']:.4f} curv {e['curv']:+.4f}")
        assert e["lag"] == lag and np.sign(e["corr"]) == pol, (kind, lag, pol, e["lag"], e["corr"])
        assert e["gap"] >= MIN_GAP, (kind, lag, pol, e["gap"])
        assert abs(e["frac"]) <= 0.5
        assert (e["frac"] == 0.0 and e["curv"] == 0.0) if abs(lag) == L else e["curv"] < 0.0
        worst = min(worst, e["gap"])
    print(f"N {N} L {L}: smallest gap {worst:.4f}")


def test_r_is_the_definition():
    """Against the plain double loop on a small row, and against numpy's full correlation."""
    rng = np.random.default_rng(5)
    d, w = rng.standard_normal(23).astype(np.float32), rng.standard_normal(23).astype(np.float32)
    L = 22
    r, s = h.xcorr64(d, w, L)
    for l in range(-L, L + 1):
        ref = sum(float(d[n]) * float(w[n + l]) for n in range(23) if 0 <= n + l < 23)
        assert abs(r[l + L] - ref) <= 1e-13
        assert s[l + L] >= abs(r[l + L])
    full = np.correlate(w.astype(np.float64), d.astype(np.float64), mode="full")     # full[k] = sum_n d[n] w[n + k - 22]
    assert np.allclose(full, r, rtol=0.0, atol=1e-13)
    r0, _ = h.xcorr64(d, w, 0)
    assert r0.shape == (1,) and r0[0] == r[L]


def test_convention_and_shift():
    """wet[n + lag] = sign(corr) dry[n]; shift64 with the estimate gives the dry row back where the index stays inside."""
    rng = np.random.default_rng(11)
    x = rng.standard_normal(300).astype(np.float32)
    for lag, pol in ((7, 1), (-4, -1), (0, -1)):
        dry = x[20:220]
        wet = (pol * x[20 - lag:220 - lag]).astype(np.float32)
        e = h.estimate64(dry, wet, 16)
        assert e["lag"] == lag and np.sign(e["corr"]) == pol
        back = h.shift64(wet[None], [e["lag"]], [e["corr"]])[0]
        lo, hi = max(0, -lag), min(200, 200 - lag)
        assert np.array_equal(back[lo:hi], dry[lo:hi])
        assert np.all(back[:lo] == 0.0) and np.all(back[hi:] == 0.0)
    w = np.arange(1, 6, dtype=np.float32)[None]
    assert np.array_equal(h.shift64(w, [2])[0], [3, 4, 5, 0, 0]) and np.array_equal(h.shift64(w, [-4])[0], [0, 0, 0, 0, 1])
    assert np.array_equal(h.shift64(w, [5])[0], np.zeros(5)) and np.array_equal(h.shift64(w, [0], [-0.5])[0], -w[0])


def test_silent_rows():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(64).astype(np.float32)
    z = np.zeros(64, dtype=np.float32)
    for dry, wet in ((z, x), (x, z), (z, z)):
        e = h.estimate64(dry, wet, 8)
        assert (e["lag"], e["corr"], e["frac"]) == (0, 0.0, 0.0)


def test_ties_by_hand():
    for dry, wet, L, lag, sign in h.tie_rows():
        e = h.estimate64(dry, wet, L)
        a = np.abs(e["c"])
        assert np.sum(a == a.max()) == 2 and e["gap"] == 0.0                  # a true tie
        assert e["lag"] == lag and np.sign(e["corr"]) == sign
        assert abs(e["corr"]) == pytest.approx(1.0 / np.sqrt(2.0), abs=1e-15)


def test_frac_finds_a_parabolas_vertex():
    """|c| sampled from a parabola with its vertex at 3.3: frac is 0.3 (the three-point formula is exact for a parabola)."""
    L = 6
    l = np.arange(-L, L + 1, dtype=np.float64)
    c = 0.9 - 0.01 * (l - 3.3) ** 2
    d = np.ones(4, dtype=np.float32)
    p = h.peak64(d, d, c * 4.0, L)                                            # sqrt(4 * 4) = 4
    assert p["lag"] == 3 and p["frac"] == pytest.approx(0.3, abs=1e-12)
    p = h.peak64(d, d, -c * 4.0, L)                                           # the same on an inverted pair
    assert p["lag"] == 3 and p["frac"] == pytest.approx(0.3, abs=1e-12) and p["corr"] < 0
    flat = np.full(2 * L + 1, 2.0)
    p = h.peak64(d, d, flat, L)                                               # all equal: lag 0, zero denominator
    assert p["lag"] == 0 and p["frac"] == 0.0

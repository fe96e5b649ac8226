"""CPU: the fp64 restatement of K26 (tests/helpers/warp64.py) against K24's helper and against itself, ``fit_lag_line`` (the
helper's and ``alignment``'s, which is host code) on hand-made tables, and the two acceptance pairs in the helper alone --
the conditions that keep the GPU tests of tests/test_gpu_warp_pairs.py from hiding a failure:

    position error of the estimated line <= 0.05 samples everywhere in the file;
    ESR of estimate-then-warp against the true wet <= 1e-4;
    ESR of the constant median lag (K19's reduction) >= 0.1.

Measured here: +300 ppm / +37.4: 0.0086 samples, 7.3e-6, 0.37;  -120 ppm / -12.3 inverted: 0.0086 samples, 2.7e-6, 0.27."""
import numpy as np
import pytest

from tests.helpers import resample64
from tests.helpers import warp64 as h


def test_taps_are_k24s_prototype():
    """At drift 0 and offset = i0 + p / up the taps are the resampler's prototype at the same tau, to the bit."""
    pl = resample64.plan(44100, 44100)
    half, T = h.plan()
    assert (pl.half, pl.taps_per_phase, pl.c) == (half, T, 0.95) == (51, 103, 0.95)
    up = 147
    for p in (0, 1, 73, 146):
        i0, f = h.positions(1, 7 + p / up, 0.0)
        assert i0[0] == 7 and f[0] == (7 + p / up) - 7
        tau = f[0] + (half - np.arange(T)).astype(np.float64)
        assert np.array_equal(h.taps(f, half)[0], resample64.prototype(tau, pl))
    assert h.taps(np.array([0.25]), half)[0, 0] == 0.0                        # tau = half + 0.25: beyond the window
    x = np.array([3.0, 64.0, -2.5, 0.0])
    assert np.array_equal(h.i0(x), np.array([resample64.i0(float(v)) for v in x]))


def test_rows_on_small_cases():
    half, T = h.plan()
    x = np.random.default_rng(1).standard_normal(400)
    y, a, ax = h.rows(x, 37.0, 0.0, n_out=300, with_bound=True)
    # an integer offset at drift 0: the band-limited copy of x[m + 37] -- white noise loses the twentieth of its power that
    # lies above 0.95 Nyquist (and half of the transition band's), so the copy is close and NOT exact
    lost = float(np.mean((y - x[37:337]) ** 2))
    assert 0.01 < lost < 0.12 and np.all(a >= np.abs(y))
    # the same row by the definition, one output at a time
    for m in (0, 17, 299):
        idx = m + 37 - half + np.arange(T)
        ok = (idx >= 0) & (idx < 400)
        want = 0.0
        for k in np.nonzero(ok)[0]:
            want += h.prototype(np.float64(half - k), half) * x[idx[k]]
        assert y[m] == want
    # outputs whose window misses the row are exact zeros; the sign negates
    z, _, zx = h.rows(x, -500.0, 1e-3, n_out=300, with_bound=True)
    assert np.all(z[zx == 0.0] == 0.0) and (zx == 0.0).sum() > 100
    assert np.array_equal(h.rows(x, 0.5, 2e-4, sign=-1.0), -h.rows(x, 0.5, 2e-4))
    two = h.rows(np.stack([x, x]), [0.5, 3.0], [2e-4, -1e-3], n_out=50)
    assert np.array_equal(two[0], h.rows(x, 0.5, 2e-4, n_out=50)) and np.array_equal(two[1], h.rows(x, 3.0, -1e-3, n_out=50))


def both():
    from mod_extraction_amd import alignment
    return (h.fit_lag_line, alignment.fit_lag_line)


@pytest.mark.parametrize("which", (0, 1))
def test_fit_lag_line_on_hand_made_tables(which):
    fit = both()[which]
    c = np.arange(16) * 8000.0 + 4095.5
    lag = 37.4 + 300e-6 * c
    corr = np.full(16, -0.9)
    p = fit(c, lag, corr)
    assert p.ok and abs(p.offset - 37.4) <= 1e-12 and abs(p.drift - 300e-6) <= 1e-12 and p.resid <= 1e-12
    assert p.polarity == -1 and p.n_probes == 16 and p.corr == 0.9
    # up to a quarter of the probes a period of 211 samples off: the medians do not move; resid names them
    moved = lag.copy()
    moved[[1, 6, 11, 14]] += np.array([211.0, -211.0, 211.0, 211.0])
    q = fit(c, moved, corr, max_resid=1e3)
    assert q.ok and abs(q.offset - 37.4) <= 1e-9 and abs(q.drift - 300e-6) <= 1e-12 and abs(q.resid - 211.0) <= 1e-6
    assert not fit(c, moved, corr).ok                                         # cause 3: a probe further than max_resid off
    off = fit(c, moved, corr)
    assert (off.offset, off.drift, off.polarity, off.n_probes) == (0.0, 0.0, 1, 16) and abs(off.resid - 211.0) <= 1e-6
    # weak and silent probes are left out of the line
    weak = corr.copy()
    weak[[0, 3]] = (0.2, 0.0)
    bent = lag.copy()
    bent[[0, 3]] += 50.0
    r = fit(c, bent, weak)
    assert r.ok and r.n_probes == 14 and abs(r.offset - 37.4) <= 1e-12 and r.resid <= 1e-12
    # cause 1: fewer than min_probes left
    few = np.where(np.arange(16) < 2, 0.9, 0.1)
    assert fit(c, lag, few) == (0.0, 0.0, 1, 0.1, 0.0, 2, False)
    assert not fit([], [], []).ok and not fit([5.0] * 4, [1.0] * 4, [0.9] * 4).ok        # nothing; no two centres apart
    # cause 2: enough strong probes on the line, and a file whose median probe is weak
    mostly = np.where(np.arange(16) < 5, 0.9, 0.1)
    m = fit(c, lag, mostly)
    assert not m.ok and m.n_probes == 5 and m.corr == 0.1 and m.resid <= 1e-12
    assert fit(c, lag, mostly, min_corr=0.05).ok
    # drift 0 with an integer offset is K19's lag
    k = fit(c, np.full(16, 5.0), np.full(16, 0.8))
    assert (k.offset, k.drift, k.polarity, k.ok) == (5.0, 0.0, 1, True)


def test_the_two_functions_agree():
    r = np.random.default_rng(4)
    for _ in range(20):
        n = int(r.integers(3, 17))
        c = np.sort(r.uniform(0, 1e5, n))
        lag = r.uniform(-50, 50) + r.uniform(-3e-4, 3e-4) * c + r.normal(0, 0.05, n)
        corr = r.uniform(0.3, 1.0, n) * r.choice([-1, 1])
        a, b = (f(c, lag, corr) for f in both())
        assert tuple(a)[2:] == tuple(b)[2:] and abs(a.offset - b.offset) <= 1e-9 and abs(a.drift - b.drift) <= 1e-13


@pytest.mark.parametrize("name", sorted(h.PAIRS))
def test_acceptance_pair_in_the_helper_alone(name):
    drift, offset, pol, extra = h.PAIRS[name]
    dry, wet = h.source()
    rec = h.recorded(name)
    assert dry.dtype == rec.dtype == np.float32 and len(dry) == h.L == 132300 and len(rec) == h.L + extra
    a = h.acceptance(name)
    line = a["line"]
    print(f"{name}: line offset {line.offset:.4f} drift {1e6 * line.drift:.3f} ppm polarity {line.polarity} resid {line.resid:.3f}; "
          f"position error {a['pos_err']:.4f} samples; ESR warp {a['esr']:.3e}, constant lag {a['median_lag']} {a['esr_const']:.3e}")
    assert line.ok and line.polarity == pol and line.n_probes == h.N_PROBES
    assert a["pos_err"] <= 0.05
    assert a["esr"] <= 1e-4
    assert a["esr_const"] >= 0.1
    # the warp at the TRUE line, on the first 20000 samples: what the interpolation alone leaves
    true = h.rows(rec, offset, drift, n_out=20000, sign=pol)
    floor = h.esr(true, wet[:20000])
    print(f"{name}: ESR of the warp at the true line {floor:.3e}")
    assert floor <= 1e-6

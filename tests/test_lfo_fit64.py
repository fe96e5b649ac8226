"""CPU: the LFO fit as a definition (include/modex_hip.h, K18), on its numpy restatement tests/helpers/lfo_fit64.py -- what
the fit finds on clean LFOs, and its special cases.  The kernel is held to the same helper in tests/test_gpu_lfo_fit.py.

Rows: ``0.1 + 0.7 t`` for the six default shapes, one rate from each of the bands 1.5-3, 3-6 and 6-12 cycles in the row (kept
inside the rate window: at 16 points the window ends at 4 cycles) and a uniform phase, all from one seeded generator; at
(n, sr, window) = (345, 172.5, 0.25-8 Hz), (48, 24, 0.25-4 Hz) and (16, 8, 0.25-2 Hz), the default grid (rate_div 4, 32 phases,
4 rounds).  Bounds: the shape is exact; the rate is within the last round's spacing df / 2^L of the true one; resid <= 1e-3;
the runner-up shape's resid is >= 1e-3 above the best (the GPU test's shape equality rests on this gap).

The refinement is a descent on an objective that is not smooth for the two saws (a jump that crosses a sample moves R by a
whole sample's worth).  On 540 rows drawn this way with seeds 0.. (12 seeds at 16 and 48 points, 6 at 345) 6 rows, all saw or
rsaw, ended in a neighbouring local minimum (shape right, rate within 3 %, resid 3e-4 .. 4e-2); the seed used here has none.
DESIGN section 7 states this with the one-cycle ambiguity.
"""
import functools

import numpy as np
import pytest

from tests.helpers import lfo_fit64 as h

SIZES = [(345, 172.5, 8.0), (48, 24.0, 4.0), (16, 8.0, 2.0)]
F_MIN, SEED = 0.25, 5
BANDS = ((1.5, 3.0), (3.0, 6.0), (6.0, 12.0))


@functools.lru_cache(maxsize=None)
def clean_fits(n, sr, f_max):
    """[(shape name, true rate, row, fit)] of the 18 clean rows of a size: fitted once, shared, not modified."""
    rng = np.random.default_rng(SEED)
    out = []
    for name in h.SHAPES[:6]:
        for lo, hi in BANDS:
            f = min(rng.uniform(lo, hi) / (n / sr), 0.95 * f_max)
            y = h.make_row(n, sr, name, f, rng.uniform(0.0, 2.0 * np.pi))
            out.append((name, f, y, h.fit_row(y, sr, F_MIN, f_max)))
    return out


@pytest.mark.parametrize("n,sr,f_max", SIZES)
def test_clean_rows_shape_rate_resid_and_gap(n, sr, f_max):
    df, L = sr / (4 * n), 4
    worst = {"rate": 0.0, "resid": 0.0, "gap": np.inf}
    for name, f, y, r in clean_fits(n, sr, f_max):
        per = np.sort(r["per_shape"])
        rel = abs(float(r["rate_hz"]) - f) / f
        worst = {"rate": max(worst["rate"], rel / (df / 2 ** L / f)), "resid": max(worst["resid"], r["resid"]),
                 "gap": min(worst["gap"], per[1] - per[0])}
        assert h.SHAPES[r["shape"]] == name, (name, f, r)
        assert rel <= df / 2 ** L / f, (name, f, r)
        assert r["resid"] <= 1e-3, (name, f, r)
        assert per[1] - per[0] >= 1e-3, (name, f, r)
        assert r["amp"] >= 0.0 and 0.0 <= float(r["phase"]) < 2.0 * np.pi
        assert abs(r["amp"] - 0.7) <= 0.05 and abs(r["offset"] - 0.1) <= 0.05
        assert np.isinf(r["per_shape"][6]) and np.isfinite(r["per_shape"][:6]).all() and int(np.argmin(r["per_shape"])) == r["shape"]
    print(f"n {n}: worst rate error {worst['rate']:.3f} of df / 2^L, worst resid {worst['resid']:.2e}, smallest gap {worst['gap']:.2e}")


def test_synth_formula_reproduces_the_best_template():
    """``offset + amp * template(rate_hz, phase, shape)`` in fp32, as ``modulations.synth_from_fit`` forms it, has against the
    row the residual the fit reports.  The fp32 roundings of offset, amp, the product and the sum move every point by at most
    e = 2^-22 (|offset| + |amp|) (four roundings, each at most 2^-24 of a value below |offset| + |amp|), so with r the fp64 residual
    vector |sqrt(sum (y - synth)^2) - sqrt(R)| <= sqrt(n) e."""
    n, sr, f_max = SIZES[1]
    for name, f, y, r in clean_fits(n, sr, f_max):
        assert h.eval_at(y, sr, r["shape"], r["rate_hz"], r["phase"])["R"] == r["R"]       # the very candidate
        d = y.astype(np.float64) - h.synth(r, n, sr).astype(np.float64)
        e = 2.0 ** -22 * (abs(r["offset"]) + abs(r["amp"]))
        assert abs(np.sqrt((d * d).sum()) - np.sqrt(r["R"])) <= np.sqrt(n) * e, (name, f)
        # the continuation: the next n points are the template at start = n, and the two pieces are one 2 n template
        both = h.template(2 * n, sr, r["shape"], r["rate_hz"], r["phase"])[0]
        assert np.array_equal(both[n:], h.template(n, sr, r["shape"], r["rate_hz"], r["phase"], start=n)[0])
        assert np.array_equal(h.synth(r, n, sr, start=n), h.F32(r["offset"]) + h.F32(r["amp"]) * both[n:])


def test_amplitude_is_never_negative():
    """1 - saw is rsaw: a negated saw is fitted AS rsaw with a positive amplitude, and with only saw allowed it is fitted
    badly (amp >= 0) rather than as saw with amp = -0.7; the same for the rectified pair."""
    n, sr = 48, 24.0
    for name, mirror in (("saw", "rsaw"), ("rsaw", "saw"), ("rect_cos", "inv_rect_cos"), ("inv_rect_cos", "rect_cos")):
        y = h.make_row(n, sr, name, 1.7, 1.0, amp=-0.7, offset=0.8)
        r = h.fit_row(y, sr, F_MIN, 4.0)
        assert h.SHAPES[r["shape"]] == mirror and r["amp"] > 0.6 and r["resid"] <= 1e-3, (name, r)
        only = h.fit_row(y, sr, F_MIN, 4.0, mask=h.mask_of([name]))
        assert h.SHAPES[only["shape"]] == name and only["amp"] >= 0.0 and only["resid"] > 0.05, (name, only)


def test_constant_row():
    y = np.full(48, 0.3, dtype=np.float32)
    r = h.fit_row(y, 24.0, F_MIN, 4.0, mask=h.mask_of(["tri", "saw"]))
    assert r["shape"] == 3 and float(r["rate_hz"]) == F_MIN and float(r["phase"]) == 0.0 and r["amp"] == 0.0
    assert r["offset"] == float(np.float32(0.3)) and r["resid"] == 0.0
    assert [float(v) for v in r["per_shape"]] == [np.inf, np.inf, np.inf, 0.0, 0.0, np.inf, np.inf]


def anti_row():
    """16 points alternating +1 / -1 against a 4-point square wave (2 Hz at 8 Hz, the four centre phases a quarter period
    apart, so no edge falls on a sample): Sty is exactly 0 at every candidate."""
    return np.asarray([1.0, -1.0] * 8, dtype=np.float32), dict(sr=8.0, f_min=2.0, f_max=2.0, mask=1 << 6, J=4, L=0)


def test_row_without_a_positive_correlation():
    y, kw = anti_row()
    r = h.fit_row(y, **kw)
    assert r["shape"] == 6 and float(r["rate_hz"]) == 2.0 and r["amp"] == 0.0 and r["resid"] == 1.0 and r["offset"] == 0.0
    # and a candidate that correlates negatively has a = 0, R = Syy
    y = h.make_row(48, 24.0, "cos", 1.5, 0.5)
    t = h.template(48, 24.0, 0, 1.5, 0.5)
    o = h.objective((1.0 - y).astype(np.float32), t)
    assert o["a"][0] == 0.0 and o["R"][0] == o["Syy"]


def test_known_rate():
    """K == 1 (f_min == f_max): phase and shape at a known rate."""
    n, sr = 48, 24.0
    assert h.grid_of(n, sr, 1.7, 1.7, 4)[4] == 1
    for name in h.SHAPES[:6]:
        y = h.make_row(n, sr, name, 1.7, 2.5)
        r = h.fit_row(y, sr, 1.7, 1.7)
        assert h.SHAPES[r["shape"]] == name and float(r["rate_hz"]) == float(np.float32(1.7)) and r["resid"] <= 1e-3, (name, r)


def test_mask_restricts_the_answer():
    n, sr = 48, 24.0
    y = h.make_row(n, sr, "tri", 1.7, 2.5)
    r = h.fit_row(y, sr, F_MIN, 4.0, mask=h.mask_of(["cos", "saw"]))
    assert r["shape"] == 0 and np.isinf(r["per_shape"][[1, 2, 3, 5, 6]]).all() and r["resid"] > 1e-3
    sq = h.fit_row(h.make_row(n, sr, "sqr", 1.7, 2.5), sr, F_MIN, 4.0, mask=0x7F)
    assert sq["shape"] == 6 and sq["resid"] <= 1e-3


def test_grid_and_phase_conventions():
    f_min, f_max, sr, df, K = h.grid_of(345, 172.5, 0.25, 8.0, 4)
    assert (df, K) == (0.125, 63)
    # the phase is the template's own argument at position (n + 1) / 2, minus the run up to it: cos has its minimum there at 0
    f32, ph32 = h.candidate(0, np.asarray([1.0]), np.asarray([0.0]), 345, 172.5)
    t = h.template(345, 172.5, 0, f32, ph32)[0]
    assert int(np.argmin(t[100:250])) + 100 == 172                         # point index 172 is position 173 = (n + 1) / 2
    for sh in range(7):
        f32, ph32 = h.candidate(sh, np.linspace(0.25, 8.0, 50), np.linspace(0.0, 6.28, 50), 345, 172.5)
        assert f32.dtype == ph32.dtype == np.float32 and (ph32 >= 0).all() and (ph32.astype(np.float64) < 2.0 * np.pi).all()

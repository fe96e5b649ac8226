"""CPU: the fp64 restatement of the rational resampler (tests/helpers/resample64.py, K24) against what it restates -- scipy's
polyphase resampler fed the same prototype, analytic sines, and exact integer arithmetic.  No device work, no library."""
from fractions import Fraction

import numpy as np
import pytest

from tests.helpers import resample64 as h

RATIOS = [(48000, 44100), (44100, 48000), (96000, 44100)]
FILTERS = [(48, 0.95, 16.0), (32, 0.95, 12.0), (16, 0.9, 8.0), (5, 1.0, 0.0)]


@pytest.mark.parametrize("sr_in, sr_out", RATIOS)
@pytest.mark.parametrize("zeros, rolloff, beta", FILTERS)
def test_rows_are_scipys_resample_poly_with_the_prototype_as_window(sr_in, sr_out, zeros, rolloff, beta):
    from scipy.signal import resample_poly
    pl = h.plan(sr_in, sr_out, zeros, rolloff, beta)
    j = np.arange(-pl.half * pl.up, pl.half * pl.up + 1, dtype=np.float64)
    proto = h.prototype(j / pl.up, pl, beta)                         # proto[j + half up] = h(j / up)
    x = np.random.default_rng(zeros).standard_normal(2000)
    want = resample_poly(x, pl.up, pl.down, window=proto / pl.up)
    got = h.rows(x, pl, table=h.taps(pl, beta))
    assert got.shape == want.shape == (pl.out_length(2000),)
    err = np.abs(got - want).max()
    print(f"{sr_in} -> {sr_out}, zeros {zeros}: max |helper - resample_poly| = {err:.2e}")
    assert err <= 1e-12 * np.abs(want).max()


def _interior(pl, n_out):
    edge = int(np.ceil((pl.half + 1) * pl.up / pl.down)) + 1
    return slice(edge, n_out - edge)


@pytest.mark.parametrize("sr_in, sr_out", [(a, b) for a in (44100, 48000, 96000) for b in (44100, 48000, 96000) if a != b])
def test_default_filter_passes_sines_to_1e_7(sr_in, sr_out):
    pl = h.plan(sr_in, sr_out)
    n_in = 4000
    table = h.taps(pl)
    worst = 0.0
    for f in (1000.0, 15000.0, 18000.0):
        x = np.sin(2 * np.pi * f * np.arange(n_in) / sr_in + 0.3)
        y = h.rows(x, pl, table=table)
        want = np.sin(2 * np.pi * f * np.arange(y.size) / sr_out + 0.3)
        sl = _interior(pl, y.size)
        assert sl.stop - sl.start > 500
        worst = max(worst, float(np.abs(y - want)[sl].max()))
    print(f"{sr_in} -> {sr_out}: interior error of 1 / 15 / 18 kHz sines {worst:.2e}")
    assert worst <= 1e-7


def test_default_filter_removes_a_tone_above_the_new_nyquist_to_1e_7():
    pl = h.plan(48000, 44100)
    x = np.sin(2 * np.pi * 24700.0 * np.arange(4000) / 48000.0 + 0.3)     # would alias to 19.4 kHz
    y = h.rows(x, pl, table=h.taps(pl))
    left = float(np.abs(y)[_interior(pl, y.size)].max())
    print(f"24.7 kHz at 48 -> 44.1 kHz leaves {left:.2e}")
    assert left <= 1e-7


def test_twenty_khz_lies_in_the_transition_band():
    """DESIGN says so: 20 kHz at 48 -> 44.1 kHz comes out a few per cent low, neither passed nor removed."""
    pl = h.plan(48000, 44100)
    x = np.sin(2 * np.pi * 20000.0 * np.arange(4000) / 48000.0)
    y = h.rows(x, pl, table=h.taps(pl))
    amp = float(np.abs(y)[_interior(pl, y.size)].max())
    assert 0.9 < amp < 0.99


@pytest.mark.parametrize("sr_in, sr_out", RATIOS)
def test_lengths_and_indices_are_exact(sr_in, sr_out):
    pl = h.plan(sr_in, sr_out)
    r = Fraction(sr_out, sr_in)
    assert Fraction(pl.up, pl.down) == r and np.gcd(pl.up, pl.down) == 1
    for n_in in range(1, 501):
        n_out = pl.out_length(n_in)
        assert n_out - 1 < n_in * r <= n_out                                   # ceil(n_in up / down)
        i0, p = h.index(np.arange(n_out), pl)
        want = [divmod(m * pl.down, pl.up) for m in range(n_out)]
        assert i0.tolist() == [w[0] for w in want] and p.tolist() == [w[1] for w in want]
        # every output starts inside the row, and the next one would not: m / sr_out < n_in / sr_in exactly for m < n_out
        assert i0.max() <= n_in - 1 and n_out * pl.down >= n_in * pl.up


def test_plan_figures():
    assert h.plan(48000, 44100)[:4] == (147, 160, 55, 111) and h.plan(48000, 44100).route == h.ROUTE_LDS
    assert h.plan(96000, 44100)[:4] == (147, 320, 110, 221) and h.plan(96000, 44100).route == h.ROUTE_LDS
    assert h.plan(44100, 48000)[:4] == (160, 147, 51, 103)
    assert h.plan(22050, 44100)[:4] == (2, 1, 51, 103)
    assert h.plan(44100, 32000)[:4] == (320, 441, 70, 141) and h.plan(44100, 32000).route == h.ROUTE_L2

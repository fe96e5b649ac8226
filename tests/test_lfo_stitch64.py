"""CPU: the numpy fp64 restatement of K22 (tests/helpers/lfo_stitch64.py) checked on its own -- what the GPU test of
``mx_lfo_stitch`` compares against.

* Windows that all sample ONE linear function a p + b of the sample position give a track equal to it at every p_j (a
  weighted mean of equal values, and linear interpolation is exact on a line): 1e-12.
* One window with L = N and n_t = n_f returns the window: 1e-15 relative (p_j falls on frame j exactly -- the helper keeps
  positions as rationals -- so the fraction is 0 and a v / a is one rounding).
* ``cover`` equals a brute-force count written here with floats-free integer comparisons of its own.
"""
import numpy as np
import pytest

from tests.helpers import lfo_stitch64 as S


def starts_of(L, N, hop):
    s = list(range(0, L - N + 1, hop))
    return s if s[-1] == L - N else s + [L - N]


CASES = [(64, 64, 64, 5), (64, 65, 32, 5), (64, 209, 16, 2), (64, 209, 64, 7), (22272, 66833, 1000, 345), (22272, 22273, 11136, 345),
         (100, 317, 37, 9)]


@pytest.mark.parametrize("N, L, hop, n_f", CASES)
def test_a_line_is_reproduced(N, L, hop, n_f):
    starts = starts_of(L, N, hop)
    a, b = 3.0e-5, -0.25
    windows = np.stack([a * S.window_positions(s, N, n_f) + b for s in starts])
    for n_t in (2, max(2, round(L * n_f / N)), 101):
        track, cover = S.stitch(windows, starts, L, N, n_t)
        assert cover.min() >= 1
        err = np.abs(track - (a * S.positions(L, n_t) + b)).max()
        print(N, L, hop, n_f, n_t, "line error", err)
        assert err <= 1e-12


@pytest.mark.parametrize("N, n_f", [(64, 2), (64, 5), (64, 64), (22272, 345), (88200, 345)])
def test_one_window_is_returned(N, n_f):
    x = np.random.default_rng(N + n_f).standard_normal((1, n_f))
    track, cover = S.stitch(x, [0], N, N, n_f)
    assert (cover == 1).all()
    err = (np.abs(track - x[0]) / np.abs(x[0])).max()
    print(N, n_f, "relative error", err)
    assert err <= 1e-15


@pytest.mark.parametrize("N, L, hop, n_f", CASES)
def test_cover_is_the_brute_force_count(N, L, hop, n_f):
    starts = starts_of(L, N, hop)
    windows = np.zeros((len(starts), n_f))
    for n_t in (2, max(2, round(L * n_f / N)), 50):
        _, cover = S.stitch(windows, starts, L, N, n_t)
        want = [sum(1 for s in starts if s * (n_t - 1) <= j * (L - 1) <= (s + N - 1) * (n_t - 1)) for j in range(n_t)]
        assert cover.tolist() == want
        assert cover[0] >= 1 and cover[-1] >= 1


def test_weights_prefer_the_window_centre():
    """Two windows that disagree by a constant: at the centre of window 0 (where window 1 has its edge) the track is window
    0's value to about 1e-3 -- the floor of the taper -- and halfway between the centres it is the plain mean."""
    N, L, hop, n_f = 64, 96, 32, 5
    windows = np.stack([np.zeros(n_f), np.ones(n_f)])
    track, cover = S.stitch(windows, [0, 32], L, N, 96)                    # p_j = j
    assert cover[31] == 1 and cover[32] == 2 and cover[63] == 2 and cover[64] == 1
    assert track[32] < 2e-3 and track[63] > 1 - 2e-3
    mid = 0.5 * (track[47] + track[48])                                    # p = 47.5: u = 0.75 and 0.25
    assert abs(mid - 0.5) <= 1e-12

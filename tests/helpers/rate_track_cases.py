"""The inputs the tests of the rate contour (K25) share: the kernel-level cases of tests/test_gpu_rate_track.py (whose CPU twin,
tests/test_rate_track64.py::test_an_ulp_on_the_nodes, runs the helper over the same rows) and the acceptance family of
tests/test_rate_track64.py (whose third row tests/test_gpu_rate_track_file.py fits on the device).  Everything is seeded, computed
once and not modified."""
import functools

import numpy as np

from tests.helpers import lfo_fit64 as h
from tests.helpers import rate_track64 as r

SIX = h.SHAPES[:6]
SR = 172.5

# name -> n, W, hop, sr, window, J, D, shapes, rows as (shape, rate, phase, amp, noise), constant span or None
CASES = {
    # K J = 252 / 256 / 260 at J = 4: one candidate tile nearly full, exactly full, and a second tile of four
    "kj252": (689, 345, 172, 172.5, (0.25, 8.0), 4, 1, ("tri",), (("tri", 1.3, 1.0, 1.0, 0.0),), None),
    "kj256": (689, 345, 172, 172.5, (0.25, 8.125), 4, 1, ("tri",), (("tri", 1.3, 1.0, 1.0, 0.0),), None),
    "kj260": (689, 345, 172, 172.5, (0.25, 8.25), 4, 2, ("tri",), (("tri", 1.3, 1.0, 1.0, 0.01),), None),
    # K = 1, hop W, a right-aligned last slice, the two rectified cosines (their phase runs at half rate), D = 0
    "k1_rect": (150, 64, 64, 31.5, (1.0, 1.0), 8, 0, ("rect_cos", "inv_rect_cos"), (("rect_cos", 1.0, 0.7, 1.0, 0.0),), None),
    # W = 16, hop 7, S = 9, D = 16 >= K = 15, six shapes, three rows (amplitudes 1 and 1e-4), a constant slice inside row 1
    "w16": (72, 16, 7, 8.0, (0.25, 2.0), 32, 16, SIX,
            (("cos", 0.8, 1.0, 1.0, 0.0), ("tri", 0.6, 2.0, 1.0, 0.0), ("saw", 1.1, 0.5, 1e-4, 0.0)), (1, 21, 37)),
    # W = 64, hop W // 2, S = 3 with the last slice five points on, J = 8, six shapes
    "w64": (101, 64, 32, 31.5, (0.25, 6.0), 8, 2, SIX, (("rsaw", 2.2, 0.3, 1.0, 0.0),), None),
    # the default grid on 345-point slices: S = 1 and S = 2
    "s1": (345, 345, 172, 172.5, (0.25, 8.0), 32, 2, ("tri",), (("tri", 1.13, 2.0, 1.0, 0.0), ("tri", 3.3, 0.7, 1e-4, 0.0)), None),
    "s2": (517, 345, 172, 172.5, (0.25, 8.0), 32, 2, ("cos", "tri"), (("cos", 0.83, 1.0, 1.0, 0.01),), None),
}
@functools.lru_cache(maxsize=None)
def case(name):
    """(rows (B, n) fp32, starts, the helper's fit of every row): seeded; shared and not modified."""
    n, W, hop, sr, window, J, D, shapes, rows, const = CASES[name]
    rng = np.random.default_rng(2700 + n + J)
    y = np.stack([h.make_row(n, sr, s, f, p, amp=a, noise=noise * a, rng=rng) for s, f, p, a, noise in rows])
    if const is not None:
        y[const[0], const[1]:const[2]] = np.float32(0.3)
    starts = r.window_starts(n, W, hop)
    ref = [r.fit(row, sr, starts, W, window[0], window[1], mask=h.mask_of(shapes), J=J, D=D) for row in y]
    return y, starts, ref


# ---- the acceptance family: 16 s rows whose rate glides ----------------------------------------
N, W, HOP, WINDOW = 2760, 345, 172, (0.25, 4.0)
FAMILY = {"tri_1.0_1.3": ("tri", 1.0, 1.3, 0.05, 27), "cos_0.8_1.0": ("cos", 0.8, 1.0, 0.05, 28),
          "tri_0.45_0.7": ("tri", 0.45, 0.7, 0.07, 2700), "tri_0.5_0.6": ("tri", 0.5, 0.6, 0.10, 2708)}


@functools.lru_cache(maxsize=None)
def family_row(name):
    """(noisy fp32 row, noise-free row, true rate at the slice centres): shared with tests/test_gpu_rate_track_file.py."""
    shape, f0, f1, noise, seed = FAMILY[name]
    y, clean, f = r.glide(N, SR, shape, f0, f1, noise=noise, rng=np.random.default_rng(seed))
    starts = r.window_starts(N, W, HOP)
    return y, clean, np.asarray([f[s:s + W].mean() for s in starts]), starts


@functools.lru_cache(maxsize=None)
def path_fit(name):
    """The helper's contour of a family row at the defaults."""
    y, _, _, starts = family_row(name)
    return r.fit(y, SR, starts, W, *WINDOW)

"""K22, the LFO track of a whole recording, restated in numpy fp64 from its definition -- no product code.

Window w (n_f points) covers the samples s_w .. s_w + N - 1 of a file of L samples; its point i sits at
s_w + i (N - 1) / (n_f - 1).  Track point j sits at p_j = j (L - 1) / (n_t - 1).  Over the windows with
s_w <= p_j <= s_w + N - 1, in ascending w:

    track[j] = sum_w a_w v_w / sum_w a_w,   cover[j] = how many
    v_w = window w interpolated linearly at p_j, (1 - f) x[i0] + f x[i0 + 1],   a_w = sin^2(pi u) + 1e-3,   u = (p_j - s_w + 0.5) / N

Positions are kept as exact rationals over the common denominator D = (n_t - 1) (N - 1) (Python ints), so which windows
cover a point and which two frames it falls between are decided without rounding; only the fraction, the weight and the
two sums are fp64.  A point nobody covers gets 0 and cover 0.
"""
import math

import numpy as np


def stitch(windows, starts, L, N, n_t):
    """windows (W, n_f) of any float dtype, starts W ints -> (track (n_t,) float64, cover (n_t,) int64)."""
    x = np.asarray(windows, dtype=np.float64)
    W, n_f = x.shape
    assert W == len(starts) and n_f >= 2 and N >= 2 and L >= N and n_t >= 2
    track, cover = np.zeros(n_t), np.zeros(n_t, dtype=np.int64)
    for j in range(n_t):
        pj_num = j * (L - 1)                                        # p_j = pj_num / (n_t - 1)
        num = den = 0.0
        for w in range(W):
            s = int(starts[w])
            rel_num = pj_num - s * (n_t - 1)                        # p_j - s_w = rel_num / (n_t - 1)
            if rel_num < 0 or rel_num > (N - 1) * (n_t - 1):
                continue
            t_num, t_den = rel_num * (n_f - 1), (n_t - 1) * (N - 1)  # frame position t = t_num / t_den in 0 .. n_f - 1
            i0 = min(t_num // t_den, n_f - 2)
            frac = (t_num - i0 * t_den) / t_den
            v = (1.0 - frac) * x[w, i0] + frac * x[w, i0 + 1]
            u = (rel_num / (n_t - 1) + 0.5) / N
            a = math.sin(math.pi * u) ** 2 + 1e-3
            num += a * v
            den += a
            cover[j] += 1
        if cover[j]:
            track[j] = num / den
    return track, cover


def positions(L, n_t):
    """p_j in fp64."""
    return np.arange(n_t, dtype=np.float64) * (L - 1) / (n_t - 1)


def window_positions(s, N, n_f):
    """The sample positions of a window's points, fp64."""
    return s + np.arange(n_f, dtype=np.float64) * (N - 1) / (n_f - 1)

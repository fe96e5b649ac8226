"""The per-clip gain match (K20, include/modex_hip.h) restated in numpy fp64, one row at a time.

    a = <y_hat, y_hat>, c = <y_hat, y>, e = <y, y>;   "ls": g = c / (a + eps);   "rms": g = sqrt((e + eps) / (a + eps))
    gain_range (lo, hi): g < lo -> lo, g > hi -> hi, flagged;   g32 = fl32(g);   z = g32 * y_hat
    backward, s = <dz, y_hat>, with the fp32 g the forward applied (an INPUT here, as it is for the kernel):
        "ls"   dy_hat = g dz + s (y - 2 g y_hat) / (a + eps)
        "rms"  dy_hat = g dz - s g y_hat / (a + eps)            a flagged row: dy_hat = g dz
"""
import math

import numpy as np

MODES = ("ls", "rms")


def gain64(a, c, e, mode, eps=1e-8, gain_range=None):
    """(g as a python float before the fp32 rounding, flag) from the three sums."""
    assert mode in MODES
    g = c / (a + eps) if mode == "ls" else float(np.sqrt((e + eps) / (a + eps)))
    flag = 0
    if gain_range is not None:
        lo, hi = gain_range
        assert 0.0 < lo <= 1.0 <= hi
        if g < lo:
            g, flag = lo, 1
        if g > hi:
            g, flag = hi, 1
    return float(g), flag


def forward64(y_hat, y, mode, eps=1e-8, gain_range=None):
    """dict for one row: ``sums`` (a, c, e), ``abs_sums`` (the sums of |terms|, what the rounding bound of an fp64 sum is stated
    in), ``g64`` (before the rounding), ``g32`` (np.float32, the applied gain), ``flag``, ``z64`` = g32 * y_hat in fp64 (the
    kernel's z is its one rounding to fp32)."""
    p, q = np.asarray(y_hat, dtype=np.float64), np.asarray(y, dtype=np.float64)
    assert p.ndim == 1 and p.shape == q.shape
    # fp32 inputs: every product is exact in fp64 and fsum adds them with one rounding, so these are the sums themselves
    a, c, e = math.fsum(p * p), math.fsum(p * q), math.fsum(q * q)
    g64, flag = gain64(a, c, e, mode, eps, gain_range)
    g32 = np.float32(g64)
    return {"sums": np.array([a, c, e]), "abs_sums": np.array([a, float(np.dot(np.abs(p), np.abs(q))), e]), "g64": g64,
            "g32": g32, "flag": flag, "z64": float(g32) * p}


def backward64(dz, y_hat, y, g32, a, flag, mode, eps=1e-8):
    """dict for one row: ``dy_hat`` fp64, ``s``, ``abs_s`` = sum |dz y_hat|, and ``scale``, per element
    |g dz| + |s y / (a + eps)| + |2 s g y_hat / (a + eps)| (the magnitudes a single fp32 rounding of dy_hat is measured in).
    ``g32``: the gain the forward applied -- the kernel's is an fp32 value; any float is taken as it is, which is how the
    finite-difference test differentiates the un-rounded function; ``a``: the forward's first sum; ``flag``: 1 = the row was
    clamped."""
    assert mode in MODES
    d, p, q = (np.asarray(v, dtype=np.float64) for v in (dz, y_hat, y))
    g = float(g32)
    s = math.fsum(d * p)
    k = 0.0 if flag else s / (a + eps)
    if mode == "ls":
        dy = g * d + k * (q - 2.0 * g * p)
    else:
        dy = g * d - (k * g) * p
    scale = np.abs(g * d) + np.abs(k * q) + np.abs(2.0 * k * g * p)
    return {"dy_hat": dy, "s": s, "abs_s": float(np.dot(np.abs(d), np.abs(p))), "scale": scale}


def rows64(y_hat, y, mode, eps=1e-8, gain_range=None):
    """``forward64`` on every row of (B, N) arrays: dict of stacked arrays (sums (B, 3), abs_sums, g64, g32, flag, z64)."""
    outs = [forward64(p, q, mode, eps, gain_range) for p, q in zip(np.asarray(y_hat), np.asarray(y))]
    return {k: np.stack([np.asarray(o[k]) for o in outs]) for k in outs[0]}


def rows_backward64(dz, y_hat, y, g32, a, flag, mode, eps=1e-8):
    """``backward64`` on every row: dict of stacked arrays (dy_hat (B, N), s, abs_s, scale (B, N))."""
    outs = [backward64(dz[b], y_hat[b], y[b], g32[b], float(a[b]), int(flag[b]), mode, eps) for b in range(len(dz))]
    return {k: np.stack([np.asarray(o[k]) for o in outs]) for k in outs[0]}

"""The lag and polarity estimate (K19, include/modex_hip.h) restated in numpy fp64: r, c, the tie rule, frac, the
zero-energy rule, the shift -- and the seeded table of dry / wet rows the CPU and GPU tests share.

    r[l + L] = sum_n dry[n] wet[n + l]  (both indices in [0, N));   c = r / sqrt(sum dry^2 sum wet^2)
    lag = argmax |c|, ties to the smallest |l|, then to l >= 0;   corr = c[lag]
    frac = 0.5 (a - c+) / (a - 2 b0 + c+) on |c| at lag - 1, lag, lag + 1; 0 at the edges or for a zero denominator
"""
import functools

import numpy as np

SIZES = ((257, 8), (4096, 64), (4099, 129))
KINDS = ("white", "pink")
POLS = (1, -1)
TAP_MIN, TAP_MAX = 5, 35


def lags_of(N, L):
    return (-L, -3, 0, 1, L)


def xcorr64(dry, wet, L):
    """(r, s): r as defined, s[l + L] = sum_n |dry[n] wet[n + l]| (what the rounding bound of an fp64 sum is stated in)."""
    d, w = np.asarray(dry, dtype=np.float64), np.asarray(wet, dtype=np.float64)
    N = d.size
    assert d.shape == w.shape == (N,) and 0 <= L < N
    r, s = np.zeros(2 * L + 1), np.zeros(2 * L + 1)
    ad, aw = np.abs(d), np.abs(w)
    for l in range(-L, L + 1):
        lo, hi = max(0, -l), min(N, N - l)
        r[l + L] = np.dot(d[lo:hi], w[lo + l:hi + l])
        s[l + L] = np.dot(ad[lo:hi], aw[lo + l:hi + l])
    return r, s


def peak64(dry, wet, r, L):
    """dict(lag, corr, frac, c, gap, curv): ``c`` the normalised row, ``gap`` the peak |c| minus the largest other |c| (inf
    with one lag), ``curv`` the parabola's denominator a - 2 b0 + c+ (0 at the edges)."""
    d, w = np.asarray(dry, dtype=np.float64), np.asarray(wet, dtype=np.float64)
    ed, ew = float(np.dot(d, d)), float(np.dot(w, w))
    if ed == 0.0 or ew == 0.0:
        return {"lag": 0, "corr": 0.0, "frac": 0.0, "c": np.zeros(2 * L + 1), "gap": 0.0, "curv": 0.0}
    c = np.asarray(r, dtype=np.float64) / np.sqrt(ed * ew)
    a = np.abs(c)
    best = 0
    for k in range(1, 2 * L + 1):
        l, lb = k - L, best - L
        if a[k] > a[best] or (a[k] == a[best] and (abs(l) < abs(lb) or (abs(l) == abs(lb) and l > lb))):
            best = k
    frac = curv = 0.0
    if 0 < best < 2 * L:
        curv = (a[best - 1] - 2.0 * a[best]) + a[best + 1]
        if curv != 0.0:
            frac = 0.5 * (a[best - 1] - a[best + 1]) / curv
    others = np.delete(a, best)
    gap = float(a[best] - others.max()) if others.size else float("inf")
    return {"lag": best - L, "corr": float(c[best]), "frac": float(frac), "c": c, "gap": gap, "curv": float(curv)}


def estimate64(dry, wet, L):
    r, s = xcorr64(dry, wet, L)
    return dict(peak64(dry, wet, r, L), r=r, s=s)


def shift64(wet, lag, corr=None):
    """out[b, n] = s_b wet[b, n + lag[b]], 0 outside the row; s_b = -1 where corr[b] < 0.  fp32 in, fp32 out."""
    wet = np.asarray(wet, dtype=np.float32)
    B, N = wet.shape
    out = np.zeros_like(wet)
    for b in range(B):
        l = int(lag[b])
        lo, hi = max(0, -l), min(N, N - l)
        if lo < hi:
            out[b, lo:hi] = wet[b, lo + l:hi + l]
        if corr is not None and corr[b] < 0:
            out[b] = -out[b]
    return out


# ---- the table: (N, L) x {white, pink} x lag x polarity ---------------------------------------------------------
def _source(kind, n, rng):
    x = rng.standard_normal(n)
    if kind == "pink":                                                        # one-pole low-pass, a = 0.9
        y = np.empty(n)
        acc = 0.0
        for i in range(n):
            acc = x[i] + 0.9 * acc
            y[i] = acc
        x = y * np.sqrt(1.0 - 0.81)
    return 0.25 * x


def _effect(x):
    """x + 0.5 x[n - d(n)], the tap's delay swinging over 5 .. 35 samples (a flanger's tap, rounded to whole samples)."""
    n = np.arange(x.size)
    d = np.rint(0.5 * (TAP_MIN + TAP_MAX) + 0.5 * (TAP_MAX - TAP_MIN) * np.sin(2.0 * np.pi * n / 211.0)).astype(np.int64)
    src = n - d
    return x + 0.5 * np.where(src >= 0, x[np.clip(src, 0, None)], 0.0)


@functools.lru_cache(maxsize=None)
def _render(N, L, kind):
    """(source, effect output) of length N + 2 L + 64, seeded by the case; both are cut from, never written to."""
    rng = np.random.default_rng(7919 * N + 31 * L + KINDS.index(kind))
    x = _source(kind, N + 2 * L + 64, rng)
    return x, _effect(x)


def make_pair(N, L, kind, lag, pol):
    """(dry, wet) fp32 of length N: wet[n + lag] = pol * effect(dry)[n], both cut from a longer render (no zeros enter)."""
    x, y = _render(N, L, kind)
    off = 64 + L                                                              # past the tap's warm-up, room for lag = -L..L
    dry = x[off:off + N].astype(np.float32)
    wet = (pol * y[off - lag:off - lag + N]).astype(np.float32)
    return dry, wet


def table():
    """The 60 cases as (N, L, kind, lag, pol)."""
    return [(N, L, kind, lag, pol) for (N, L) in SIZES for kind in KINDS for lag in lags_of(N, L) for pol in POLS]


def tie_rows(N=64):
    """Two hand-made ties, exact in any arithmetic: (dry, wet, L, lag, sign of corr).  A unit impulse against two impulses:
    |c| is 1 / sqrt(2) at both lags."""
    d = np.zeros(N, dtype=np.float32)
    d[30] = 1.0
    w1 = np.zeros(N, dtype=np.float32)
    w1[28] = w1[32] = 1.0                                                     # |c| equal at l = -2 and +2: the non-negative one
    w2 = np.zeros(N, dtype=np.float32)
    w2[27], w2[31] = 1.0, -1.0                                                # |c| equal at l = -3 and +1: the smaller |l|
    return [(d, w1, 5, 2, 1), (d, w2, 5, 1, -1)]

"""numpy fp64 restatement of K27 (mod_extraction_amd/csrc/shaper_match_abi.h has the definition): one polynomial curve per
clip that carries a re-render onto a recorded wet, every stage of the forward and of the backward for ONE row.  The elementwise
stages perform the kernel's operations in the kernel's order (numpy rounds every operation on its own, as the kernels do without
contraction), the sums are plain fp64 sums; ``*_abs`` are the sums of the absolute values of the same terms, which the tests'
gates are made of.  No torch, no device."""
import math

import numpy as np

CHUNK = 2048
MAX_ORDER = 7


def powers(order, even=False):
    return tuple(p for p in range(1, order + 1) if even or p % 2)


def moment_orders(order, even=False):
    p = powers(order, even)
    return tuple(sorted({a + b for a in p for b in p}))


def n_sums(order, even=False):
    return 1 + len(moment_orders(order, even)) + len(powers(order, even)) + 1


def scale(x):
    """(S2, r, bad): r = fl32(sqrt(S2 / N)) as fp64; bad: S2 or r not positive or not finite (then r = 1)."""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        S2 = float(np.sum(x * x))
        r = float(np.float32(math.sqrt(S2 / x.size))) if S2 >= 0.0 and math.isfinite(S2) else float("nan")
    bad = not (S2 > 0.0 and math.isfinite(S2) and r > 0.0 and math.isfinite(r))
    return S2, (1.0 if bad else r), bad


def _pows(t, top):
    """[t^0, t^1, .. t^top], each the one before times t"""
    out = [np.ones_like(t), t]
    for _ in range(2, top + 1):
        out.append(out[-1] * t)
    return out


def sums(x, y, order, even=False, r=None):
    """(sums, sums_abs) in the kernel's layout: S2, the moments in ascending m, b_1 .. b_K, E.  ``r``: the scale to use (the
    kernel's own, when a test checks this stage alone); None: ``scale(x)``."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    S2, r0, _ = scale(x)
    r = r0 if r is None else float(r)
    t, yr = x / r, y / r
    pw = _pows(t, 2 * order)
    val, mag = [S2], [S2]
    for m in moment_orders(order, even):
        val.append(float(np.sum(pw[m])))
        mag.append(float(np.sum(np.abs(pw[m]))))
    for p in powers(order, even):
        val.append(float(np.sum(pw[p] * yr)))
        mag.append(float(np.sum(np.abs(pw[p] * yr))))
    E = float(np.sum(y * y))
    return np.array(val + [E]), np.array(mag + [E])


def gram(s, order, even=False, ridge=0.0):
    """(A, b) from a row of sums: A[i][j] = M_(p_i + p_j), the diagonal times (1 + ridge)."""
    p, mo = powers(order, even), moment_orders(order, even)
    K = len(p)
    M = {m: s[1 + i] for i, m in enumerate(mo)}
    A = np.array([[M[p[i] + p[j]] * ((1.0 + ridge) if i == j else 1.0) for j in range(K)] for i in range(K)])
    return A, np.array(s[1 + len(mo):1 + len(mo) + K], np.float64)


def cholesky_solve(A, rhs):
    """(A^-1 rhs, pivots) by the kernel's Cholesky; None for the solution when a pivot is not positive or not finite."""
    K = len(rhs)
    L, piv = np.zeros((K, K)), []
    for j in range(K):
        d = A[j][j]
        for k in range(j):
            d -= L[j][k] * L[j][k]
        piv.append(float(d))
        if not (d > 0.0 and math.isfinite(d)):
            return None, piv
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, K):
            a = A[i][j]
            for k in range(j):
                a -= L[i][k] * L[j][k]
            L[i][j] = a / L[j][j]
    x = np.array(rhs, np.float64)
    for i in range(K):
        a = x[i]
        for k in range(i):
            a -= L[i][k] * x[k]
        x[i] = a / L[i][i]
    for i in range(K - 1, -1, -1):
        a = x[i]
        for k in range(i + 1, K):
            a -= L[k][i] * x[k]
        x[i] = a / L[i][i]
    return x, piv


def solve(s, N, order, even=False, ridge=1e-9, max_gain=20.0, round32=True):
    """(c, r, flag, pivots) from a row of sums -- the solve kernel.  ``round32=False`` keeps c in fp64 (the finite differences)."""
    K = len(powers(order, even))
    ident = np.array([1.0] + [0.0] * (K - 1))
    S2 = float(s[0])
    with np.errstate(all="ignore"):
        r = float(np.float32(math.sqrt(S2 / N))) if S2 >= 0.0 and math.isfinite(S2) else float("nan")
    if not (S2 > 0.0 and math.isfinite(S2) and r > 0.0 and math.isfinite(r)):
        return ident, 1.0, 1, []
    A, b = gram(s, order, even, ridge)
    c, piv = cholesky_solve(A, b)
    if c is None:
        return ident, r, 1, piv
    if round32:
        c = c.astype(np.float32).astype(np.float64)
    if not (float(np.sum(np.abs(c.astype(np.float32).astype(np.float64)))) <= max_gain):
        return ident, r, 2, piv
    return c, r, 0, piv


def curve(t, c, order, even=False):
    """C(t) by the kernel's Horner: with ``even`` t (c_1 + t (c_2 + ..)), else t (c_1 + s (c_3 + ..)), s = t t."""
    s = t if even else t * t
    h = np.full_like(t, c[-1])
    for k in range(len(c) - 2, -1, -1):
        h = c[k] + s * h
    return t * h


def apply(x, c, r, order, even=False, flag=0):
    """z in fp64 BEFORE the one rounding to fp32 (a flagged row: x itself)."""
    x = np.asarray(x, np.float64)
    if flag:
        return x.copy()
    return r * curve(x / r, np.asarray(c, np.float64), order, even)


def forward(x, y, order=5, even=False, ridge=1e-9, max_gain=20.0, round32=True):
    """dict(z (fp64, unrounded), c, r, sums, sums_abs, flag, pivots) of one row."""
    s, mag = sums(x, y, order, even)
    c, r, flag, piv = solve(s, len(x), order, even, ridge, max_gain, round32)
    return dict(z=apply(x, c, r, order, even, flag), c=c, r=r, sums=s, sums_abs=mag, flag=flag, pivots=piv)


def bwd_sums(dz, x, r, order, even=False):
    """(g, g_abs): g_k = sum dz t^(p_k)"""
    t = np.asarray(x, np.float64) / r
    d = np.asarray(dz, np.float64)
    pw = _pows(t, order)
    p = powers(order, even)
    return np.array([float(np.sum(d * pw[q])) for q in p]), np.array([float(np.sum(np.abs(d * pw[q]))) for q in p])


def bwd_solve(g, s, order, even=False, ridge=1e-9, flag=0):
    """u = A^-1 g (0 on a flagged row)"""
    if flag:
        return np.zeros(len(g))
    u, _ = cholesky_solve(gram(s, order, even, ridge)[0], g)
    return np.zeros(len(g)) if u is None else u


def bwd_apply(dz, x, y, c, r, u, order, even=False, ridge=1e-9, flag=0):
    """(dy_hat in fp64 before the one rounding, the sum of the absolute values of its terms) -- the kernel's operations"""
    d, x, y = (np.asarray(a, np.float64) for a in (dz, x, y))
    if flag:
        return d.copy(), np.abs(d)
    t, yr = x / r, y / r
    p = powers(order, even)
    pw = _pows(t, 2 * p[-1] - 1)
    Ct, Cd, Ut, Ud, R = (np.zeros_like(t) for _ in range(5))
    mag = np.zeros_like(t)
    aC, aCd, aU, aUd = (np.zeros_like(t) for _ in range(4))
    for k, pk in enumerate(p):
        cp, up = pk * c[k], pk * u[k]
        w = (2.0 * ridge) * (u[k] * cp)
        Ct = Ct + c[k] * pw[pk]
        Cd = Cd + cp * pw[pk - 1]
        Ut = Ut + u[k] * pw[pk]
        Ud = Ud + up * pw[pk - 1]
        R = R + w * pw[2 * pk - 1]
        aC, aCd = aC + np.abs(c[k] * pw[pk]), aCd + np.abs(cp * pw[pk - 1])
        aU, aUd = aU + np.abs(u[k] * pw[pk]), aUd + np.abs(up * pw[pk - 1])
        mag = mag + np.abs(w * pw[2 * pk - 1])
    out = ((d * Cd + Ud * yr) - (Ud * Ct + Ut * Cd)) - R
    mag = mag + np.abs(d) * aCd + aUd * np.abs(yr) + aUd * aC + aU * aCd
    return out, mag


def backward(dz, x, y, fwd, order, even=False, ridge=1e-9):
    """dict(dy (fp64, unrounded), dy_abs, g, g_abs, u) from ``forward``'s dict"""
    g, g_abs = bwd_sums(dz, x, fwd["r"], order, even)
    u = bwd_solve(g, fwd["sums"], order, even, ridge, fwd["flag"])
    dy, mag = bwd_apply(dz, x, y, fwd["c"], fwd["r"], u, order, even, ridge, fwd["flag"])
    return dict(dy=dy, dy_abs=mag, g=g, g_abs=g_abs, u=u)


def esr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sum((a - b) ** 2) / np.sum(b * b))


def ls_gain_esr(x, y):
    """the ESR the best single gain leaves"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return esr(x * (np.dot(x, y) / np.dot(x, x)), y)


def comb(n, seed, amp=1.0):
    """a noise-driven comb x[n] + 0.7 x[n - 37] at peak ``amp``, fp32"""
    w = np.random.default_rng(seed).standard_normal(n + 37)
    x = w[37:] + 0.7 * w[:-37] if n > 0 else w[:0]
    return (x * (amp / np.max(np.abs(x)))).astype(np.float32)

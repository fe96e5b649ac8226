"""The per-clip FIR match (K21, include/modex_hip.h) restated in numpy fp64, one row at a time and one stage at a time.

    x = y_hat, y: N samples, zero outside [0, N);  K taps, a centre c
    sums      R[d] = sum_n x[n] x[n + d],  b[j] = sum_n x[n + c - j] y[n],  E = sum_n y[n]^2
    solve     A = toeplitz(R) + (eps + ridge R[0]) I,  h = A^-1 b by Cholesky;  flag 1: a pivot that is not positive or not
              finite;  flag 2: not (sum |h| <= max_gain);  a flagged row: h[c] = 1, the rest 0;  taps = fl32(h)
    apply     z[n] = sum_k taps[k] x[n + c - k]
    bwd_sums  gh[k] = sum_n dz[n] x[n + c - k]
    bwd_solve u = A^-1 gh;  s[d] = sum_{k - j = d} (h[k] u[j] + u[k] h[j]), d = -(K-1) .. K-1;  s[0] += 2 ridge <u, h>;
              a flagged row: u = 0, s = 0
    bwd_apply dy_hat[i] = sum_k h[k] dz[i + k - c] + sum_k u[k] y[i + k - c] - sum_d s[d] x[i + d]

The stage functions take taps / u / s (and the sums) as ARGUMENTS, as the kernels do, so a kernel stage can be checked on the
kernel's own inputs.  ``forward64`` / ``backward64`` are the composition; with ``round_taps=False`` the taps stay fp64, which
is the function the finite-difference test differentiates.
"""
import math

import numpy as np


def shifted(v, o, N=None):
    """a[n] = v[n + o] for n in [0, N), 0 where n + o leaves [0, len(v))."""
    v = np.asarray(v, dtype=np.float64)
    N = len(v) if N is None else N
    a = np.zeros(N)
    lo, hi = max(0, -o), min(N, len(v) - o)
    if hi > lo:
        a[lo:hi] = v[lo + o:hi + o]
    return a


def fsum(t):
    """math.fsum; a vector with a non-finite term (which fsum may refuse) is added plainly: inf or NaN as IEEE gives it."""
    t = np.asarray(t, dtype=np.float64)
    if np.isfinite(t).all():
        return math.fsum(t)
    with np.errstate(all="ignore"):
        return float(np.sum(t))


def sums(x, y, K, c):
    """dict: ``sums`` (2K + 1,) = R, b, E, exact (math.fsum of exact products of fp32 values), and ``abs_sums``, the sums of the
    terms' magnitudes (what the rounding bound of an fp64 sum is stated in)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    assert x.ndim == 1 and x.shape == y.shape and 0 <= c < K
    with np.errstate(invalid="ignore"):
        terms = [x * shifted(x, d) for d in range(K)] + [shifted(x, c - j) * y for j in range(K)] + [y * y]
    return {"sums": np.array([fsum(t) for t in terms]), "abs_sums": np.array([float(np.abs(t).sum()) for t in terms])}


def system(R, ridge, eps):
    """A = toeplitz(R) + (eps + ridge R[0]) I."""
    R = np.asarray(R, dtype=np.float64)
    K = len(R)
    idx = np.abs(np.arange(K)[:, None] - np.arange(K)[None, :])
    with np.errstate(invalid="ignore"):                             # a non-finite R[0] (flag 1) times the identity's zeros
        return R[idx] + (eps + ridge * R[0]) * np.eye(K)


def cholesky(A):
    """(L, ok): the lower factor column by column; ok = False at the first pivot that is not positive or not finite."""
    K = len(A)
    L = np.zeros((K, K))
    with np.errstate(all="ignore"):
        for j in range(K):
            d = A[j, j] - np.dot(L[j, :j], L[j, :j])
            if not (d > 0.0) or not np.isfinite(d):
                return L, False
            L[j, j] = math.sqrt(d)
            for i in range(j + 1, K):
                L[i, j] = (A[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    return L, True


def chol_solve(L, r):
    K = len(r)
    w = np.zeros(K)
    for i in range(K):
        w[i] = (r[i] - np.dot(L[i, :i], w[:i])) / L[i, i]
    v = np.zeros(K)
    for i in range(K - 1, -1, -1):
        v[i] = (w[i] - np.dot(L[i + 1:, i], v[i + 1:])) / L[i, i]
    return v


def solve(sums_, K, c, ridge=1e-6, eps=1e-8, max_gain=20.0, round_taps=True):
    """dict from the row's sums (R, b, E): ``h64`` (before the rounding; the identity on a flagged row), ``taps`` (fp32, or
    h64 itself with round_taps=False), ``flag``, ``cond`` = cond_2(A) (inf where A is not finite)."""
    sums_ = np.asarray(sums_, dtype=np.float64)
    R, b = sums_[:K], sums_[K:2 * K]
    A = system(R, ridge, eps)
    L, ok = cholesky(A)
    flag, h = 0, None
    if not ok:
        flag = 1
    else:
        with np.errstate(all="ignore"):
            h = chol_solve(L, b)
            if not (np.abs(h).sum() <= max_gain):
                flag = 2
    if flag:
        h = np.zeros(K)
        h[c] = 1.0
    cond = float(np.linalg.cond(A)) if np.isfinite(A).all() else math.inf
    return {"h64": h, "taps": h.astype(np.float32) if round_taps else h.copy(), "flag": flag, "cond": cond}


def apply(x, taps, c):
    """dict: ``z64`` = sum_k taps[k] x[n + c - k] in fp64 (the kernel's z is its one rounding) and ``scale`` = the sum of the
    terms' magnitudes per sample.  A zero tap reads nothing."""
    x = np.asarray(x, dtype=np.float64)
    z, scale = np.zeros(len(x)), np.zeros(len(x))
    for k, h in enumerate(np.asarray(taps, dtype=np.float64)):
        if h != 0.0:
            t = h * shifted(x, c - k)
            z += t
            scale += np.abs(t)
    return {"z64": z, "scale": scale}


def bwd_sums(dz, x, K, c):
    """dict: ``gh`` (K,) exact and ``abs_gh``."""
    dz, x = np.asarray(dz, dtype=np.float64), np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        terms = [dz * shifted(x, c - k) for k in range(K)]
    return {"gh": np.array([fsum(t) for t in terms]), "abs_gh": np.array([float(np.abs(t).sum()) for t in terms])}


def bwd_solve(gh, R, taps, flag, ridge=1e-6, eps=1e-8):
    """dict: ``u`` (K,) and ``s`` (2K - 1,), s[K - 1 + d] for lag d; both 0 on a flagged row.  ``taps``: the h the forward
    applied (the kernel's are fp32 values; any float is taken as it is)."""
    h = np.asarray(taps, dtype=np.float64)
    K = len(h)
    if flag:
        return {"u": np.zeros(K), "s": np.zeros(2 * K - 1)}
    L, ok = cholesky(system(R, ridge, eps))
    assert ok, "an unflagged row has a factor"
    u = chol_solve(L, np.asarray(gh, dtype=np.float64))
    s = np.correlate(h, u, "full") + np.correlate(u, h, "full")       # correlate(a, v, "full")[K - 1 + d] = sum_j a[j + d] v[j]
    s[K - 1] += 2.0 * ridge * float(np.dot(u, h))
    return {"u": u, "s": s}


def bwd_apply(dz, y, x, taps, u, s, c):
    """dict: ``dy_hat`` fp64 and ``scale`` = the sum of the terms' magnitudes per sample.  Zero coefficients read nothing."""
    dz, y, x = (np.asarray(v, dtype=np.float64) for v in (dz, y, x))
    K = len(taps)
    out, scale = np.zeros(len(x)), np.zeros(len(x))
    for coefs, v, first in ((taps, dz, -c), (u, y, -c), (-np.asarray(s, dtype=np.float64), x, -(K - 1))):
        for k, a in enumerate(np.asarray(coefs, dtype=np.float64)):
            if a != 0.0:
                t = a * shifted(v, first + k)
                out += t
                scale += np.abs(t)
    return {"dy_hat": out, "scale": scale}


def forward64(x, y, K, c, ridge=1e-6, eps=1e-8, max_gain=20.0, round_taps=True):
    """The composition for one row: the dicts of ``sums``, ``solve`` and ``apply`` merged."""
    out = sums(x, y, K, c)
    out.update(solve(out["sums"], K, c, ridge, eps, max_gain, round_taps))
    out.update(apply(x, out["taps"], c))
    return out


def backward64(dz, x, y, fwd, c, ridge=1e-6, eps=1e-8):
    """d loss / d x for one row from ``fwd`` = what ``forward64`` returned: the dicts of the three backward stages merged."""
    K = len(fwd["taps"])
    out = bwd_sums(dz, x, K, c)
    out.update(bwd_solve(out["gh"], fwd["sums"][:K], fwd["taps"], fwd["flag"], ridge, eps))
    out.update(bwd_apply(dz, y, x, fwd["taps"], out["u"], out["s"], c))
    return out


def rows64(x, y, K, c, ridge=1e-6, eps=1e-8, max_gain=20.0):
    """``forward64`` on every row of (B, N) arrays: dict of stacked arrays."""
    outs = [forward64(p, q, K, c, ridge, eps, max_gain) for p, q in zip(np.asarray(x), np.asarray(y))]
    return {k: np.stack([np.asarray(o[k]) for o in outs]) for k in outs[0]}


def rows_backward64(dz, x, y, fwd, c, ridge=1e-6, eps=1e-8):
    """``backward64`` on every row, ``fwd`` = what ``rows64`` returned: dict of stacked arrays."""
    outs = [backward64(dz[b], x[b], y[b], {k: v[b] for k, v in fwd.items()}, c, ridge, eps) for b in range(len(dz))]
    return {k: np.stack([np.asarray(o[k]) for o in outs]) for k in outs[0]}

"""fp64 adjoint of the flanger / chorus driven by a LOW-RATE LFO row, TEST INFRASTRUCTURE ONLY.

The data path hands the flanger kernel an LFO of n_mod < N points and the kernel resamples it per sample
(align_corners=True, csrc/common.h interp_tap + interp_combine).  This module is tests/helpers/flanger_adjoint64.py at
full rate, composed with that resampling and its transpose:

  taps(n_mod, N)            the taps i0 / i1 and weights lam0 / lam1 of every sample, in numpy float32 in exactly interp_tap's
                            sequence: scale = (n_mod - 1) / (N - 1) as float32, real = scale * i, truncation, clamps;
  upsample32(mod_lr, N)     the fp32 LFO value of every sample, fma(lam0, x[i0], lam1 * x[i1]) correctly rounded (the slots of
                            the fp32 bookkeeping follow from these values);
  interp_transpose64(g, n)  the transpose of the resampling: sum over the samples of weight * g, in fp64;
  flanger_adjoint64_lr      the full-rate adjoint at upsample32(mod_lr), with dmod reduced to (B, n_mod).
"""
import numpy as np

from tests.helpers.flanger_adjoint64 import flanger_adjoint64

F32 = np.float32


def taps(n_mod, N):
    """i0, i1 (N,) int64 and lam0, lam1 (N,) float32 of csrc/common.h interp_tap for every output sample."""
    scale = F32(n_mod - 1) / F32(N - 1) if N > 1 else F32(0.0)          # interp_scale_host
    real = (scale * np.arange(N).astype(F32)).astype(F32)
    i0 = np.minimum(real.astype(np.int64), n_mod - 1)                   # (int)real truncates; real >= 0
    lam1 = np.clip((real - i0.astype(F32)).astype(F32), F32(0.0), F32(1.0))
    i1 = i0 + (i0 < n_mod - 1)
    lam0 = (F32(1.0) - lam1).astype(F32)
    return i0, i1, lam0, lam1


def _fma32(a, b, c):
    """Correctly rounded float32 a * b + c.  The product is exact in float64; the float64 sum is corrected with its
    rounding error (TwoSum) where it lands exactly between two float32 values."""
    s = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    t = s + c
    bb = t - s
    e = (s - (t - bb)) + (c - bb)
    r = t.astype(F32)
    r64 = r.astype(np.float64)
    other = np.where(t > r64, np.nextafter(r, F32(np.inf)), np.nextafter(r, F32(-np.inf)))
    tie = (e != 0) & (t != r64) & (np.abs(t - r64) == np.abs(other.astype(np.float64) - t))
    return np.where(tie, np.where(e > 0, np.maximum(r, other), np.minimum(r, other)), r).astype(F32)


def upsample32(mod_lr, N):
    """(B, n_mod) float32 -> (B, N) float32: what the kernel's in-kernel resampling yields, bit for bit."""
    mod_lr = np.asarray(mod_lr, F32)
    n_mod = mod_lr.shape[1]
    if n_mod == N:
        return mod_lr
    i0, i1, lam0, lam1 = taps(n_mod, N)
    x0, x1 = mod_lr[:, i0], mod_lr[:, i1]
    return _fma32(np.broadcast_to(lam0, x0.shape), x0, (lam1[None, :] * x1).astype(F32))


def upsample64(mod_lr64, N):
    """The same linear map in fp64 (fp32 taps and weights, fp64 products and sums): what the adjoint differentiates."""
    n_mod = mod_lr64.shape[1]
    if n_mod == N:
        return mod_lr64
    i0, i1, lam0, lam1 = taps(n_mod, N)
    return lam0.astype(np.float64) * mod_lr64[:, i0] + lam1.astype(np.float64) * mod_lr64[:, i1]


def interp_transpose64(g_full, n_mod):
    """(B, N) -> (B, n_mod) fp64: the transpose of upsample64."""
    g = np.asarray(g_full, np.float64)
    B, N = g.shape
    if n_mod == N:
        return g
    i0, i1, lam0, lam1 = taps(n_mod, N)
    out = np.zeros((B, n_mod))
    for b in range(B):
        np.add.at(out[b], i0, lam0.astype(np.float64) * g[b])
        np.add.at(out[b], i1, lam1.astype(np.float64) * g[b])
    return out


def flanger_adjoint64_lr(x, mod_lr, consts, M, dy, mod_full=None):
    """flanger_adjoint64 for a low-rate LFO: "dmod" is (B, n_mod); "dmod_full" the per-sample gradient it was reduced from,
    "mod_full" the fp32 per-sample LFO (``mod_full`` overrides upsample32, e.g. with the kernel's own mod_up output)."""
    x = np.asarray(x)
    mod_lr = np.asarray(mod_lr, F32)
    full = upsample32(mod_lr, x.shape[1]) if mod_full is None else np.asarray(mod_full, F32)
    out = flanger_adjoint64(x, full, consts, M, dy)
    out["dmod_full"] = out["dmod"]
    out["dmod"] = interp_transpose64(out["dmod_full"], mod_lr.shape[1])
    out["mod_full"] = full
    return out

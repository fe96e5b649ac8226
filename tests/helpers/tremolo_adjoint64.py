"""fp64 forward and adjoint of the tremolo (fx.py:13-22) behind the align_corners=True resampling, TEST INFRASTRUCTURE ONLY.

  y[n] = (omm + mix m[n]) x[n],   m = upsample(mod)   (mod (B, n_mod), 1 <= n_mod <= N; n_mod == N: m = mod)

taps(n_mod, N) builds the interpolation taps from the definition behind util.py:15-29 (F.interpolate, mode="linear",
align_corners=True): source position real = scale * n with scale = (n_mod - 1) / (N - 1), i0 = min(floor(real), n_mod - 1),
i1 = min(i0 + 1, n_mod - 1), weights 1 - lam and lam = clamp(real - i0, 0, 1) -- evaluated in float32 in aten's sequence
(scale as a float32 quotient, real as a float32 product), because the weights the kernels use are those float32 numbers.
Everything after the taps is float64: the linear map, the products and the sums."""
import numpy as np

F32 = np.float32


def taps(n_mod, N):
    """i0, i1 (N,) int64 and lam0, lam1 (N,) float32 of every output sample."""
    scale = F32(n_mod - 1) / F32(N - 1) if N > 1 else F32(0.0)
    real = (scale * np.arange(N).astype(F32)).astype(F32)
    i0 = np.minimum(real.astype(np.int64), n_mod - 1)
    lam1 = np.clip((real - i0.astype(F32)).astype(F32), F32(0.0), F32(1.0))
    i1 = np.minimum(i0 + 1, n_mod - 1)
    return i0, i1, (F32(1.0) - lam1).astype(F32), lam1


def upsample64(mod, N):
    mod = np.asarray(mod, np.float64)
    n_mod = mod.shape[1]
    if n_mod == N:
        return mod
    i0, i1, lam0, lam1 = taps(n_mod, N)
    return lam0.astype(np.float64) * mod[:, i0] + lam1.astype(np.float64) * mod[:, i1]


def upsample_transpose64(g, n_mod):
    """(B, N) -> (B, n_mod): the transpose of upsample64."""
    g = np.asarray(g, np.float64)
    B, N = g.shape
    if n_mod == N:
        return g
    i0, i1, lam0, lam1 = taps(n_mod, N)
    out = np.zeros((B, n_mod))
    for b in range(B):
        np.add.at(out[b], i0, lam0.astype(np.float64) * g[b])
        np.add.at(out[b], i1, lam1.astype(np.float64) * g[b])
    return out


def tremolo_forward64(x, mod, mix, omm=None):
    """x (B, N), mod (B, n_mod), mix (B,) [, omm (B,): 1 - mix as the caller rounded it; default 1 - mix in fp64]."""
    x, mix = np.asarray(x, np.float64), np.asarray(mix, np.float64)
    omm = 1.0 - mix if omm is None else np.asarray(omm, np.float64)
    m = upsample64(mod, x.shape[1])
    return (omm[:, None] + mix[:, None] * m) * x


def tremolo_adjoint64(x, mod, mix, dy, omm=None):
    """Gradients of sum(y * dy): dx (B, N), dmod (B, n_mod) and dmix (B,), the latter with omm = 1 - mix differentiated
    too (d omm / d mix = -1), whatever rounded value of omm the forward used."""
    x, mix, dy = np.asarray(x, np.float64), np.asarray(mix, np.float64), np.asarray(dy, np.float64)
    omm = 1.0 - mix if omm is None else np.asarray(omm, np.float64)
    m = upsample64(mod, x.shape[1])
    p = dy * x
    return {"y": (omm[:, None] + mix[:, None] * m) * x,
            "dx": dy * (omm[:, None] + mix[:, None] * m),
            "dmod": upsample_transpose64(mix[:, None] * p, np.asarray(mod).shape[1]),
            "dmix": (p * (m - 1.0)).sum(1),
            "mod_full": m}

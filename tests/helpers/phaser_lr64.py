"""fp64 expand and gather between a low-rate LFO row and the phaser's cut-off-update grid, TEST INFRASTRUCTURE ONLY.

The phaser kernels read their external LFO once per 4 SOURCE samples, counted from the start of the source row, lead-in
included; a low-rate row of n_mod points spans the N samples of the clip window (align_corners=True).  So group g of a row
with ``lead`` lead-in samples reads the row resampled at clip sample

    n(g) = clamp(4 g - lead, 0, N - 1)        for g < ceil((lead + N) / 4);   groups beyond hold 0.5

(the LFO is held at its first value through the lead-in).  The taps are those of util.py:15-29 (F.interpolate,
mode="linear", align_corners=True), restated here in float32 in aten's sequence -- scale = float32(n_mod - 1) /
float32(N - 1), real = scale * n as a float32 product, i0 = min(int(real), n_mod - 1), lam1 = clamp(real - i0, 0, 1),
lam0 = 1 - lam1, i1 = min(i0 + 1, n_mod - 1) -- because the weights the kernels use are those float32 numbers.  n_mod == N
is a plain read.  Everything after the taps is float64."""
import numpy as np

F32 = np.float32


def group_samples(N, lead, n_groups):
    """(n (n_groups,) int64: the clip sample every group reads, valid (n_groups,) bool: g < ceil((lead + N) / 4))."""
    g = np.arange(n_groups, dtype=np.int64)
    return np.clip(4 * g - int(lead), 0, N - 1), g < (int(lead) + N + 3) // 4


def taps_at(n, n_mod, N):
    """i0, i1 int64 and lam0, lam1 float32 of the clip samples ``n``."""
    n = np.asarray(n, np.int64)
    if n_mod == N:
        return n, n, np.ones(n.shape, F32), np.zeros(n.shape, F32)
    scale = F32(n_mod - 1) / F32(N - 1) if N > 1 else F32(0.0)
    real = (scale * n.astype(F32)).astype(F32)
    i0 = np.minimum(real.astype(np.int64), n_mod - 1)
    lam1 = np.clip((real - i0.astype(F32)).astype(F32), F32(0.0), F32(1.0))
    return i0, np.minimum(i0 + 1, n_mod - 1), (F32(1.0) - lam1).astype(F32), lam1


def expand64(mod_lr, lead, N, width):
    """mod_lr (B, n_mod), lead (B,) ints -> (B, ceil(width / 4)) float64."""
    mod_lr = np.asarray(mod_lr, np.float64)
    B, n_mod = mod_lr.shape
    ng = (width + 3) // 4
    out = np.full((B, ng), 0.5)
    for b in range(B):
        n, valid = group_samples(N, lead[b], ng)
        i0, i1, lam0, lam1 = taps_at(n, n_mod, N)
        row = lam0.astype(np.float64) * mod_lr[b, i0] + lam1.astype(np.float64) * mod_lr[b, i1]
        out[b, valid] = row[valid]
    return out


def gather64(dmod_g, lead, N, n_mod):
    """The transpose of expand64: dmod_g (B, n_groups) -> (B, n_mod) float64 (groups beyond the clip contribute nothing)."""
    dmod_g = np.asarray(dmod_g, np.float64)
    B, ng = dmod_g.shape
    out = np.zeros((B, n_mod))
    for b in range(B):
        n, valid = group_samples(N, lead[b], ng)
        i0, i1, lam0, lam1 = taps_at(n, n_mod, N)
        d = np.where(valid, dmod_g[b], 0.0)
        np.add.at(out[b], i0, lam0.astype(np.float64) * d)
        np.add.at(out[b], i1, lam1.astype(np.float64) * d)
    return out

"""Independent references of the first Spectral2DCNN block on the f16x3 route and of the head, written from the ABI text of
include/modex_hip.h and the reference semantics it cites (LayerNorm -> Conv2d(2, 64, (5, 13), same) -> + bias ->
MaxPool2d((2, 1)); LayerNorm / PReLU backward; PReLU -> mean over bins -> Conv1d(C, L, 1) -> sigmoid) with numpy only: no
torch, no autograd, no product code.  Everything computes in float64 unless said otherwise; tests/test_block1_refs64.py holds
each function to torch's fp64 autograd.

Layouts (the ABI's):
* k-vector operand  xk[b][h][w][k = kh * 2 + ci] = xhat[b][ci][h + kh - 2][w], zero outside the image, for w >= Wv and for
  k >= 10: (B, H, 352, 16);
* k-vector weights  wk[kw][khalf][co][j] = W[co][ci][kh][kw] * 256 with k = khalf * 8 + j = kh * 2 + ci, zero for k >= 10:
  (13, 2, 64, 8);
* f16x3 pair of a value v: hi = fp16(v), lo = fp16(v - hi); packed word = hi | lo << 16 (fp16 bit patterns).
"""
import numpy as np

PITCH = 352                      # floats per row of an activation plane
KH, KW, CO = 5, 13, 64
WSCALE = 256.0                   # the weight operand carries W * 256


# ---- f16x3 pairs -------------------------------------------------------------------------------------------------------
def split16(v):
    """v (taken as float32) -> (hi, lo) float16: hi = fp16(v), lo = fp16(v - hi); v - hi is exact in fp32."""
    v32 = np.asarray(v, np.float32)
    hi = v32.astype(np.float16)
    lo = (v32 - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def pack_pair(hi, lo):
    """(hi, lo) float16 -> uint32 words hi | lo << 16."""
    h = np.ascontiguousarray(hi, np.float16).view(np.uint16).astype(np.uint32)
    l = np.ascontiguousarray(lo, np.float16).view(np.uint16).astype(np.uint32)
    return h | (l << np.uint32(16))


def unpack_pair(words):
    """uint32 words -> (hi, lo) float16."""
    w = np.ascontiguousarray(words).view(np.uint32)
    return (w & np.uint32(0xFFFF)).astype(np.uint16).view(np.float16), (w >> np.uint32(16)).astype(np.uint16).view(np.float16)


# ---- layouts -----------------------------------------------------------------------------------------------------------
def kvec_layout(xhat, Wv):
    """xhat (B, 2, H, >= Wv) -> xk (B, H, 352, 16) of xhat's dtype."""
    xhat = np.asarray(xhat)
    B, C, H = xhat.shape[:3]
    assert C == 2
    xk = np.zeros((B, H, PITCH, 16), xhat.dtype)
    for kh in range(KH):
        for ci in range(2):
            for h in range(H):
                src = h + kh - 2
                if 0 <= src < H:
                    xk[:, h, :Wv, kh * 2 + ci] = xhat[:, ci, src, :Wv]
    return xk


def kvec_weights(W, scale=WSCALE):
    """W (64, 2, 5, 13) -> (13, 2, 64, 8) float64 of W * scale."""
    W = np.asarray(W, np.float64)
    wk = np.zeros((KW, 2, CO, 8))
    for kh in range(KH):
        for ci in range(2):
            k = kh * 2 + ci
            wk[:, k // 8, :, k % 8] = W[:, ci, kh, :].T * scale
    return wk


# ---- the first block ---------------------------------------------------------------------------------------------------
def plane_stats(x, eps=1e-5):
    """x (B, C, H, W) -> (B, C, 2) = {mean, 1 / sqrt(biased variance + eps)} per plane."""
    x = np.asarray(x, np.float64)
    mean = x.mean((2, 3))
    var = ((x - mean[:, :, None, None]) ** 2).mean((2, 3))
    return np.stack([mean, 1.0 / np.sqrt(var + eps)], -1)


def normalise(x, stats):
    """(x - mean) * rstd with stats (B, C, 2) taken as given (e.g. the fp32 values a kernel is handed)."""
    st = np.asarray(stats, np.float64)
    return (np.asarray(x, np.float64) - st[:, :, 0, None, None]) * st[:, :, 1, None, None]


def conv1(xhat, W):
    """z[b][co][h][w] = sum over (ci, kh, kw) of W[co][ci][kh][kw] xhat[b][ci][h + kh - 2][w + kw - 6], zero outside the
    image (torch's Conv2d, padding "same", no bias).  The loop over the 65 taps gathers the shifted images; the sum over
    (ci, tap) is one fp64 matrix product per clip."""
    xhat, W = np.asarray(xhat, np.float64), np.asarray(W, np.float64)
    B, C, H, Wd = xhat.shape
    xp = np.zeros((B, C, H + KH - 1, Wd + KW - 1))
    xp[:, :, 2:2 + H, 6:6 + Wd] = xhat
    Wm = W.reshape(W.shape[0], C * KH * KW)
    z = np.empty((B, W.shape[0], H, Wd))
    col = np.empty((C, KH, KW, H, Wd))
    for b in range(B):
        for kh in range(KH):
            for kw in range(KW):
                col[:, kh, kw] = xp[b, :, kh:kh + H, kw:kw + Wd]
        z[b] = (Wm @ col.reshape(C * KH * KW, H * Wd)).reshape(-1, H, Wd)
    return z


def pool21(z):
    """MaxPool2d((2, 1)): (pooled, amax uint8), amax = 1 iff the odd row is GREATER than the even row (ties: the even row)."""
    even, odd = z[:, :, 0::2], z[:, :, 1::2]
    amax = odd > even
    return np.where(amax, odd, even), amax.astype(np.uint8)


def conv1_pool_fwd(xhat, W, bias):
    """-> (out (B, 64, H / 2, W) = pooled z + bias, amax, z without the bias)."""
    z = conv1(xhat, W)
    pooled, amax = pool21(z)
    return pooled + np.asarray(bias, np.float64)[None, :, None, None], amax, z


def route(G, amax):
    """G, amax (B, 64, H / 2, W) -> dz (B, 64, H, W): G on the row the argmax names, zero on the other."""
    G = np.asarray(G, np.float64)
    B, C, Hp, Wd = G.shape
    dz = np.zeros((B, C, 2 * Hp, Wd))
    dz[:, :, 0::2] = np.where(np.asarray(amax) == 0, G, 0.0)
    dz[:, :, 1::2] = np.where(np.asarray(amax) == 1, G, 0.0)
    return dz


def conv1_wgrad(dz, xhat):
    """dW[co][ci][kh][kw] = sum over (b, h, w) of dz[b][co][h][w] xhat[b][ci][h + kh - 2][w + kw - 6]."""
    dz, xhat = np.asarray(dz, np.float64), np.asarray(xhat, np.float64)
    B, C, H, Wd = xhat.shape
    xp = np.zeros((B, C, H + KH - 1, Wd + KW - 1))
    xp[:, :, 2:2 + H, 6:6 + Wd] = xhat
    dW = np.zeros((dz.shape[1], C, KH, KW))
    for kh in range(KH):
        for kw in range(KW):
            dW[:, :, kh, kw] = np.tensordot(dz, xp[:, :, kh:kh + H, kw:kw + Wd], axes=([0, 2, 3], [0, 2, 3]))
    return dW


def prelu(v, slope):
    """v > 0 ? v : slope v (+0 and -0 take the slope branch)."""
    return np.where(v > 0, v, slope * v)


def stats_rows(out, bias, slope):
    """The forward kernel's optional by-product: (B, H, 64, 2) = {sum, sum of squares} over the columns of
    d = PReLU(out) - PReLU(bias), and the sums of magnitudes {sum (|PReLU(out)| + |PReLU(bias)|), sum of its square}."""
    out = np.asarray(out, np.float64)
    sl, b = np.asarray(slope, np.float64)[None, :, None, None], np.asarray(bias, np.float64)[None, :, None, None]
    y, sh = prelu(out, sl), prelu(b, sl)
    d, m = y - sh, np.abs(y) + np.abs(sh)
    tr = lambda a: a.sum(-1).transpose(0, 2, 1)
    return np.stack([tr(d), tr(d * d)], -1), np.stack([tr(m), tr(m * m)], -1)


# ---- LayerNorm + PReLU backward ------------------------------------------------------------------------------------------
def ln_prelu_bwd(p, dxhat, stats, slope, m12=None):
    """p, dxhat (B, C, H, W); x = PReLU(p), xhat = (x - mean) rstd, dx = rstd (dxhat - m1 - xhat m2) with m1 = mean(dxhat),
    m2 = mean(dxhat xhat) over the plane (or m12 = (m1, m2), each (B, C), as given); G = dx (p > 0 ? 1 : slope).
    Returns dict(G, dslope (B, C) = sum dx p [p <= 0], gsum (B, C) = sum G, m1, m2, xhat, and the magnitudes G_mag
    (elementwise sum of the magnitudes of G's terms), dslope_mag, gsum_mag)."""
    p, g = np.asarray(p, np.float64), np.asarray(dxhat, np.float64)
    st = np.asarray(stats, np.float64)
    sl = np.asarray(slope, np.float64)[None, :, None, None]
    mean, rstd = st[:, :, 0, None, None], st[:, :, 1, None, None]
    x = prelu(p, sl)
    xh = (x - mean) * rstd
    if m12 is None:
        m1, m2 = g.mean((2, 3)), (g * xh).mean((2, 3))
    else:
        m1, m2 = (np.asarray(m, np.float64) for m in m12)
    m1b, m2b = m1[:, :, None, None], m2[:, :, None, None]
    dx = rstd * (g - m1b - xh * m2b)
    fac = np.where(p > 0, 1.0, sl)
    G = dx * fac
    xh_mag = (np.abs(x) + np.abs(mean)) * rstd
    dx_mag = rstd * (np.abs(g) + np.abs(m1b) + xh_mag * np.abs(m2b))
    ds = np.where(p > 0, 0.0, dx * p)
    return dict(G=G, dslope=ds.sum((2, 3)), gsum=G.sum((2, 3)), m1=m1, m2=m2, xhat=xh, G_mag=dx_mag * np.abs(fac),
                dslope_mag=np.where(p > 0, 0.0, dx_mag * np.abs(p)).sum((2, 3)), gsum_mag=(dx_mag * np.abs(fac)).sum((2, 3)))


# ---- head --------------------------------------------------------------------------------------------------------------
def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-np.asarray(v, np.float64)))


def head_fwd(p6, slope, wout, bout):
    """p6 (B, C, Hl, W), slope (C,), wout (L, C), bout (L,) -> dict(latent (B, C, W) = mean over bins of PReLU(p6),
    pre (B, L, W), out = sigmoid(pre), and latent_mag = mean |PReLU(p6)|, pre_mag = sum |wout| |latent| + |bout|)."""
    p6 = np.asarray(p6, np.float64)
    y = prelu(p6, np.asarray(slope, np.float64)[None, :, None, None])
    latent = y.mean(2)
    w, b = np.asarray(wout, np.float64), np.asarray(bout, np.float64)
    pre = np.einsum("lc,bcw->blw", w, latent) + b[None, :, None]
    pre_mag = np.einsum("lc,bcw->blw", np.abs(w), np.abs(latent)) + np.abs(b)[None, :, None]
    return dict(latent=latent, pre=pre, out=sigmoid(pre), latent_mag=np.abs(y).mean(2), pre_mag=pre_mag)


def head_bwd(p6, slope, wout, latent, out, d_out, d_latent):
    """dlogit = d_out out (1 - out); dlat = d_latent (None: 0) + sum_l wout[l][c] dlogit[l]; dy = dlat / Hl on every bin;
    G6 = dy (p6 > 0 ? 1 : slope); per-clip partials dwout (B, L, C) = sum_w dlogit latent, dbout (B, L) = sum_w dlogit,
    dslope (B, C) = sum dy p6 [p6 <= 0].  Returns them with the magnitudes G6_mag, dwout_mag, dbout_mag, dslope_mag."""
    p6, w = np.asarray(p6, np.float64), np.asarray(wout, np.float64)
    lat, o, do = np.asarray(latent, np.float64), np.asarray(out, np.float64), np.asarray(d_out, np.float64)
    sl = np.asarray(slope, np.float64)[None, :, None, None]
    Hl = p6.shape[2]
    dlogit = do * o * (1.0 - o)
    dl = np.zeros_like(lat) if d_latent is None else np.asarray(d_latent, np.float64)
    dlat = dl + np.einsum("lc,blw->bcw", w, dlogit)
    dlat_mag = np.abs(dl) + np.einsum("lc,blw->bcw", np.abs(w), np.abs(dlogit))
    dy, dy_mag = (dlat / Hl)[:, :, None, :], (dlat_mag / Hl)[:, :, None, :]
    fac = np.where(p6 > 0, 1.0, sl)
    return dict(G6=dy * fac, G6_mag=dy_mag * np.abs(fac), dlogit=dlogit,
                dwout=np.einsum("blw,bcw->blc", dlogit, lat), dwout_mag=np.einsum("blw,bcw->blc", np.abs(dlogit), np.abs(lat)),
                dbout=dlogit.sum(-1), dbout_mag=np.abs(dlogit).sum(-1),
                dslope=np.where(p6 > 0, 0.0, dy * p6).sum((2, 3)), dslope_mag=np.where(p6 > 0, 0.0, dy_mag * np.abs(p6)).sum((2, 3)))

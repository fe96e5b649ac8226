"""Independent references of the "general" kernels (mx_sgemm_f32, the im2col / col2im gathers, the row / channel / plane
normalisations, pool + PReLU, the bin-mean head, FiLM, the mx_lstmg_* recurrence), written from the definitions in
include/modex_hip.h with numpy only: no torch, no product, no oracle, so no formula is shared with what they check.

Every elementwise and recurrence reference computes in ``dtype`` (default float64).  With ``dtype=np.float32`` the same
formulae run in fp32: the yardstick of what plain fp32 arithmetic costs on the same inputs (used where an error compounds
and cannot be derived).  The reductions the kernels keep in fp64 (row_sums, chan_stats, the ``part`` / ``dgb`` sums) are always
fp64 here and return the sum of the magnitudes of their terms beside the value.
"""
import numpy as np

PITCH = 352                      # floats per row of the TCN activation planes (B, C, 352)


# ---- mx_sgemm_f32: the ABI's addressing on flat buffers ------------------------------------------------------------------
def sgemm(a, a_off, a_rs, a_cs, a_bs, b, b_off, b_rs, b_cs, b_bs, c, c_off, c_rs, c_cs, c_bs, M, N, K, n_batch,
          batches_per_group, accumulate):
    """C[m c_rs + n c_cs] (+)= sum_k A[m a_rs + k a_cs] B[k b_rs + n b_cs]; batch i reads a + i a_bs / b + i b_bs, group
    g = i // batches_per_group sums its batches and writes c + g c_bs.  a, b, c: flat arrays, *_off: element offset of the
    base pointer.  Returns (c_out float64 flat, written bool flat, mag float64 flat = sum |A||B| (+ |C_in|) per written
    element, summed int flat = batches summed into each written element)."""
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    c_out = np.asarray(c, np.float64).ravel().copy()
    written = np.zeros(c_out.size, bool)
    mag = np.zeros(c_out.size)
    summed = np.zeros(c_out.size, np.int64)
    m, n, k = np.arange(M), np.arange(N), np.arange(K)
    ai = a_off + m[:, None] * a_rs + k[None, :] * a_cs
    bi = b_off + k[:, None] * b_rs + n[None, :] * b_cs
    ci = c_off + m[:, None] * c_rs + n[None, :] * c_cs
    groups = -(-n_batch // batches_per_group)
    for g in range(groups):
        acc, am, cnt = np.zeros((M, N)), np.zeros((M, N)), 0
        for i in range(g * batches_per_group, min(n_batch, (g + 1) * batches_per_group)):
            A, Bm = a[ai + i * a_bs], b[bi + i * b_bs]
            acc += A @ Bm
            am += np.abs(A) @ np.abs(Bm)
            cnt += 1
        idx = ci + g * c_bs
        assert np.unique(idx).size == idx.size and not written[idx].any(), "the C layout aliases itself"
        if accumulate:
            acc = acc + c_out[idx]
            am = am + np.abs(c_out[idx])
        c_out[idx], mag[idx], written[idx], summed[idx] = acc, am, True, cnt
    return c_out, written, mag, summed


# ---- mx_im2col2d / mx_col2im2d ----------------------------------------------------------------------------------------
def same_pad(k, d):
    """aten's padding="same": total = d (k - 1), floor(total / 2) before, the remainder after."""
    return d * (k - 1) // 2


def im2col2d(x, kh, kw, dh, dw, pt, pl):
    """x (nb, Cin, H, W) -> col (Cin kh kw, nb H W): col[(ci kh + i) kw + j][(b H + h) W + w] = x[b][ci][h + i dh - pt]
    [w + j dw - pl], 0 outside the image."""
    nb, Cin, H, W = x.shape
    col = np.zeros((Cin, kh, kw, nb, H, W), x.dtype)
    for i in range(kh):
        for j in range(kw):
            oh, ow = i * dh - pt, j * dw - pl                       # source = destination + (oh, ow)
            h0, h1 = max(0, -oh), min(H, H - oh)
            w0, w1 = max(0, -ow), min(W, W - ow)
            if h0 < h1 and w0 < w1:
                col[:, i, j, :, h0:h1, w0:w1] = x[:, :, h0 + oh:h1 + oh, w0 + ow:w1 + ow].transpose(1, 0, 2, 3)
    return col.reshape(Cin * kh * kw, nb * H * W)


def col2im2d(dcol, nb, Cin, H, W, kh, kw, dh, dw, pt, pl):
    """The transpose of im2col2d: every dcol element is added to the image element it was gathered from."""
    d = dcol.reshape(Cin, kh, kw, nb, H, W)
    dx = np.zeros((nb, Cin, H, W), dcol.dtype)
    for i in range(kh):
        for j in range(kw):
            oh, ow = i * dh - pt, j * dw - pl
            h0, h1 = max(0, -oh), min(H, H - oh)
            w0, w1 = max(0, -ow), min(W, W - ow)
            if h0 < h1 and w0 < w1:
                dx[:, :, h0 + oh:h1 + oh, w0 + ow:w1 + ow] += d[:, i, j, :, h0:h1, w0:w1].transpose(1, 0, 2, 3)
    return dx


# ---- mx_tcn_im2col / mx_tcn_col2im ------------------------------------------------------------------------------------
def conv1d_out_len(T, ksz, dilation, stride):
    """nn.Conv1d's output length with padding = (ksz // 2) dilation (tcn.py)."""
    return (T + 2 * (ksz // 2) * dilation - dilation * (ksz - 1) - 1) // stride + 1


def tcn_im2col(x, stats, T, To, ksz, dilation, stride, dtype=np.float64):
    """x (B, C, 352) planes, T valid columns; stats (B, 2) = {mean, rstd} or None -> col (C ksz, B To):
    col[ci ksz + k][b To + t'] = xhat[b][ci][t' stride + (k - ksz // 2) dilation], 0 outside [0, T)."""
    x = np.asarray(x, dtype)
    B, C = x.shape[:2]
    xh = x[:, :, :T]
    if stats is not None:
        st = np.asarray(stats, dtype).reshape(B, 2)
        xh = (xh - st[:, 0, None, None]) * st[:, 1, None, None]
    col = np.zeros((C, ksz, B, To), dtype)
    for k in range(ksz):
        for t in range(To):
            src = t * stride + (k - ksz // 2) * dilation
            if 0 <= src < T:
                col[:, k, :, t] = xh[:, :, src].T
    return col.reshape(C * ksz, B * To)


def tcn_col2im(dcol, B, C, T, To, ksz, dilation, stride):
    """The transpose of tcn_im2col (without statistics): dx (B, C, T)."""
    d = dcol.reshape(C, ksz, B, To)
    dx = np.zeros((B, C, T), dcol.dtype)
    for k in range(ksz):
        for t in range(To):
            src = t * stride + (k - ksz // 2) * dilation
            if 0 <= src < T:
                dx[:, :, src] += d[:, k, :, t].T
    return dx


# ---- sums ---------------------------------------------------------------------------------------------------------------
def row_sums(x):
    """(rows, n) -> (sum, sum of magnitudes) of every row, in fp64."""
    x = np.asarray(x, np.float64)
    return x.sum(-1), np.abs(x).sum(-1)


# ---- nn.LayerNorm over one contiguous row, no affine -------------------------------------------------------------------
def rowln_fwd(x, eps, dtype=np.float64):
    """x (rows, n) -> y = (x - mean) rstd, stats (rows, 2) = {mean, rstd}; biased variance, eps inside the root."""
    x = np.asarray(x, dtype)
    mean = x.mean(-1, keepdims=True, dtype=dtype)
    var = ((x - mean) ** 2).mean(-1, keepdims=True, dtype=dtype)
    rstd = (1.0 / np.sqrt(var + dtype(eps))).astype(dtype)
    return (x - mean) * rstd, np.concatenate([mean, rstd], -1)


def rowln_bwd(dy, y, stats, dtype=np.float64):
    """dx = rstd (dy - mean(dy) - y mean(dy y)); also returns the two means (m1, m2), each (rows, 1)."""
    dy, y = np.asarray(dy, dtype), np.asarray(y, dtype)
    rstd = np.asarray(stats, dtype)[:, 1:2]
    m1 = dy.mean(-1, keepdims=True, dtype=dtype)
    m2 = (dy * y).mean(-1, keepdims=True, dtype=dtype)
    return rstd * (dy - m1 - y * m2), (m1, m2)


# ---- TCN planes (B, C, 352), T valid columns ---------------------------------------------------------------------------
def prelu(v, slope):
    """nn.PReLU: v > 0 ? v : slope v (so +0 and -0 take the slope branch)."""
    return np.where(v > 0, v, slope * v)


def tcn_act_fwd(z, bias, slope, res, T, dtype=np.float64):
    """z (B, C, 352): zb = z + bias on [0, T); y = PReLU(zb; slope[c]) (slope None: identity) + res (None: none), zero on
    [T, 352).  Returns (zb (B, C, T), y (B, C, 352))."""
    z = np.asarray(z, dtype)
    B, C = z.shape[:2]
    zb = z[:, :, :T] + (0 if bias is None else np.asarray(bias, dtype)[None, :, None])
    out = zb if slope is None else prelu(zb, np.asarray(slope, dtype)[None, :, None])
    if res is not None:
        out = out + np.asarray(res, dtype)[:, :, :T]
    y = np.zeros((B, C, PITCH), dtype)
    y[:, :, :T] = out
    return zb, y


def tcn_act_bwd(dy, zb, slope, T, dtype=np.float64):
    """dz = dy (zb > 0 ? 1 : slope[c]) on [0, T), zero on [T, 352); part (B C, 2) = {sum dz, sum dy zb [zb <= 0]} (the second is
    0 without a slope).  Returns (dz, part, part_mag)."""
    dy, zb = np.asarray(dy, dtype)[:, :, :T], np.asarray(zb, dtype)[:, :, :T]
    B, C = dy.shape[:2]
    a = np.ones(C, dtype) if slope is None else np.asarray(slope, dtype)
    g = np.where(zb > 0, dy, a[None, :, None] * dy)
    sl = np.where(zb > 0, 0, dy * zb) if slope is not None else np.zeros_like(dy)
    dz = np.zeros((B, C, PITCH), dtype)
    dz[:, :, :T] = g
    part = np.stack([g.sum(-1), sl.sum(-1)], -1).reshape(B * C, 2)
    mag = np.stack([np.abs(g).sum(-1), np.abs(sl).sum(-1)], -1).reshape(B * C, 2)
    return dz, part, mag


def tcn_ln_bwd(x, dxhat, stats, add, T, dtype=np.float64):
    """LayerNorm([C, T]) backward per clip: dx = rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat)) + add on [0, T), zero
    on [T, 352).  Returns (dx, (m1, m2), xhat)."""
    x, g = np.asarray(x, dtype)[:, :, :T], np.asarray(dxhat, dtype)[:, :, :T]
    B, C = x.shape[:2]
    st = np.asarray(stats, dtype).reshape(B, 2)
    mean, rstd = st[:, 0, None, None], st[:, 1, None, None]
    xh = (x - mean) * rstd
    m1 = g.mean((1, 2), keepdims=True, dtype=dtype)
    m2 = (g * xh).mean((1, 2), keepdims=True, dtype=dtype)
    v = rstd * (g - m1 - xh * m2)
    if add is not None:
        v = v + np.asarray(add, dtype)[:, :, :T]
    dx = np.zeros((B, C, PITCH), dtype)
    dx[:, :, :T] = v
    return dx, (m1, m2), xh


# ---- Conv2d bias + MaxPool2d((p, 1)) + PReLU -----------------------------------------------------------------------------
def pool_prelu_fwd(z, bias, C, p, slope, dtype=np.float64):
    """z (planes, H, W), channel of a plane = plane % C.  v = maximum over each window of p rows of z + bias[c] (rows beyond
    (H // p) p dropped), amax = offset of the FIRST maximum, out = PReLU(v; slope[c])."""
    z = np.asarray(z, dtype)
    planes, H, W = z.shape
    Hp = H // p
    ch = np.arange(planes) % C
    zb = z[:, :Hp * p] + np.asarray(bias, dtype)[ch, None, None]
    win = zb.reshape(planes, Hp, p, W)
    amax = win.argmax(2)                                          # numpy: the first occurrence
    v = np.take_along_axis(win, amax[:, :, None, :], 2)[:, :, 0, :]
    return v, prelu(v, np.asarray(slope, dtype)[ch, None, None]), amax.astype(np.uint8)


def pool_prelu_bwd(g, v, amax, C, H, p, slope, dtype=np.float64):
    """d = g (v > 0 ? 1 : slope[c]) routed to row amax of its window, zero elsewhere (dropped rows included); part
    (planes, 2) = {sum d, sum g v [v <= 0]}.  Returns (dz (planes, H, W), part, part_mag)."""
    g, v = np.asarray(g, dtype), np.asarray(v, dtype)
    planes, Hp, W = g.shape
    ch = np.arange(planes) % C
    d = np.where(v > 0, g, np.asarray(slope, dtype)[ch, None, None] * g)
    sl = np.where(v > 0, 0, g * v)
    dz = np.zeros((planes, H, W), dtype)
    win = dz[:, :Hp * p].reshape(planes, Hp, p, W)
    np.put_along_axis(win, np.asarray(amax, np.int64)[:, :, None, :], d[:, :, None, :], 2)
    dz[:, :Hp * p] = win.reshape(planes, Hp * p, W)
    part = np.stack([d.sum((1, 2)), sl.sum((1, 2))], -1)
    mag = np.stack([np.abs(d).sum((1, 2)), np.abs(sl).sum((1, 2))], -1)
    return dz, part, mag


# ---- head: mean over bins -> Conv1d(C, L, 1) -> sigmoid ------------------------------------------------------------------
def sigmoid(v):
    """1 / (1 + exp(-v)) in v's own precision (the constants take v's dtype: no promotion to fp64)."""
    v = np.asarray(v)
    one = v.dtype.type(1)
    return one / (one + np.exp(-v))


def binmean_head_fwd(x, wout, bout, dtype=np.float64):
    """x (B, C, H, W), wout (L, C), bout (L,) -> latent (B, C, W), out (B, L, W), pre (B, L, W) (the Conv1d output)."""
    x = np.asarray(x, dtype)
    latent = x.sum(2, dtype=dtype) / dtype(x.shape[2])
    pre = np.einsum("lc,bcw->blw", np.asarray(wout, dtype), latent) + np.asarray(bout, dtype)[None, :, None]
    return latent, sigmoid(pre).astype(dtype), pre


def binmean_head_bwd(d_out, d_latent, out, wout, B, C, H, W, dtype=np.float64):
    """ds = d_out out (1 - out) (0 without d_out); dx = (d_latent + sum_l wout[l][c] ds[l]) / H on every bin.
    Returns (ds (B, L, W), dx (B, C, H, W), mag (B, C, W) = sum of the magnitudes of dx's terms, before the division)."""
    out, wout = np.asarray(out, dtype), np.asarray(wout, dtype)
    ds = np.zeros_like(out) if d_out is None else np.asarray(d_out, dtype) * out * (1 - out)
    dl = np.zeros((B, C, W), dtype) if d_latent is None else np.asarray(d_latent, dtype)
    tot = dl + np.einsum("lc,blw->bcw", wout, ds)
    mag = np.abs(dl) + np.einsum("lc,blw->bcw", np.abs(wout), np.abs(ds))
    dx = np.broadcast_to((tot / dtype(H))[:, :, None, :], (B, C, H, W)).copy()
    return ds, dx, mag


# ---- per-channel pieces of the general TCN: (B, C, T) dense ---------------------------------------------------------------
def chan_stats(z):
    """(B, C, T) -> stats (C, 2) = {mean, biased variance} over (clips, frames) in fp64, and the sums of magnitudes behind them."""
    z = np.asarray(z, np.float64)
    mean = z.mean((0, 2))
    d = z - mean[None, :, None]
    n = z.shape[0] * z.shape[2]
    return np.stack([mean, (d * d).mean((0, 2))], -1), np.stack([np.abs(z).sum((0, 2)) / n, (d * d).sum((0, 2)) / n], -1)


def chan_norm_fwd(z, norm, dtype=np.float64):
    z, norm = np.asarray(z, dtype), np.asarray(norm, dtype)
    return (z - norm[None, :, 0, None]) * norm[None, :, 1, None]


def chan_norm_bwd(g, xhat, norm, train, dtype=np.float64):
    """train: dz = rstd (g - mean(g) - xhat mean(g xhat)) with the means over (clips, frames); eval: dz = rstd g.
    Returns (dz, (m1, m2))."""
    g, xhat = np.asarray(g, dtype), np.asarray(xhat, dtype)
    rstd = np.asarray(norm, dtype)[None, :, 1, None]
    if not train:
        return rstd * g, (np.zeros((1, g.shape[1], 1), dtype),) * 2
    m1 = g.mean((0, 2), keepdims=True, dtype=dtype)
    m2 = (g * xhat).mean((0, 2), keepdims=True, dtype=dtype)
    return rstd * (g - m1 - xhat * m2), (m1, m2)


def film_fwd(xhat, gb, dtype=np.float64):
    """a = xhat gain + shift, gb (B, 2 C) = [gain | shift]."""
    xhat, gb = np.asarray(xhat, dtype), np.asarray(gb, dtype)
    C = xhat.shape[1]
    return xhat * gb[:, :C, None] + gb[:, C:, None]


def film_bwd(da, xhat, gb, dtype=np.float64):
    """dxhat = da gain (in ``dtype``); dgb (B, 2 C) = [sum da xhat | sum da] over frames (fp64).  Returns (dxhat, dgb, dgb_mag)."""
    C = np.asarray(xhat).shape[1]
    dxhat = np.asarray(da, dtype) * np.asarray(gb, dtype)[:, :C, None]
    da, xhat = np.asarray(da, np.float64), np.asarray(xhat, np.float64)
    dgb = np.concatenate([(da * xhat).sum(-1), da.sum(-1)], -1)
    mag = np.concatenate([np.abs(da * xhat).sum(-1), np.abs(da).sum(-1)], -1)
    return dxhat, dgb, mag


def prelu_res_fwd(a, slope, res, dtype=np.float64):
    a = np.asarray(a, dtype)
    y = a if slope is None else prelu(a, np.asarray(slope, dtype)[None, :, None])
    return y if res is None else y + np.asarray(res, dtype)


def prelu_res_bwd(dy, a, slope, dtype=np.float64):
    """da = dy (a > 0 ? 1 : slope[c]) (in ``dtype``); part (B C,) = sum over frames of dy a where a <= 0 (fp64).
    Returns (da, part, part_mag)."""
    da = np.where(np.asarray(a) > 0, np.asarray(dy, dtype), np.asarray(slope, dtype)[None, :, None] * np.asarray(dy, dtype))
    dy, a = np.asarray(dy, np.float64), np.asarray(a, np.float64)
    sl = np.where(a > 0, 0, dy * a)
    return da, sl.sum(-1).ravel(), np.abs(sl).sum(-1).ravel()


# ---- generic LSTM recurrence (gate order i, f, g, o) ---------------------------------------------------------------------
def lstmg_fwd(zin, bias_ih, bias_hh, w_hh, h0, c0, dtype=np.float64):
    """zin (B, T, 4 Hn) = W_ih u_t; gates = act(zin + bias_ih + bias_hh + W_hh h), c = f c + i g, h = o tanh(c).
    Returns (stash (B, T, 6, Hn) = (i, f, g, o, c, h) of every step, h1, c1)."""
    zin, w = np.asarray(zin, dtype), np.asarray(w_hh, dtype)
    bi, bh = np.asarray(bias_ih, dtype), np.asarray(bias_hh, dtype)
    h, c = np.asarray(h0, dtype).copy(), np.asarray(c0, dtype).copy()
    B, T, G = zin.shape
    Hn = G // 4
    stash = np.zeros((B, T, 6, Hn), dtype)
    for t in range(T):
        pre = zin[:, t] + bi + bh + h @ w.T
        i, f, o = sigmoid(pre[:, :Hn]), sigmoid(pre[:, Hn:2 * Hn]), sigmoid(pre[:, 3 * Hn:])
        g = np.tanh(pre[:, 2 * Hn:3 * Hn])
        c = f * c + i * g
        h = o * np.tanh(c)
        for q, val in enumerate((i, f, g, o, c, h)):
            stash[:, t, q] = val
    return stash, h.astype(dtype), c.astype(dtype)


def lstmg_bwd(stash, dhfc, w_hh, c0, dtype=np.float64):
    """BPTT inside the chunk from dhfc (B, T, Hn) = d loss / d h_t; the incoming state is a constant.
    Returns dgate (B, T, 4 Hn) = d loss / d gate pre-activations."""
    st, dhfc, w = np.asarray(stash, dtype), np.asarray(dhfc, dtype), np.asarray(w_hh, dtype)
    c0 = np.asarray(c0, dtype)
    B, T, _, Hn = st.shape
    dgate = np.zeros((B, T, 4 * Hn), dtype)
    dh, dc = np.zeros((B, Hn), dtype), np.zeros((B, Hn), dtype)
    one = dtype(1)
    for t in range(T - 1, -1, -1):
        i, f, g, o, c = (st[:, t, q] for q in range(5))
        cp = st[:, t - 1, 4] if t > 0 else c0
        dht = dhfc[:, t] + dh
        tc = np.tanh(c)
        dct = dc + dht * o * (one - tc * tc)
        d = np.concatenate([dct * g * i * (one - i), dct * cp * f * (one - f), dct * i * (one - g * g),
                            dht * tc * o * (one - o)], -1)
        dgate[:, t] = d
        dc = dct * f
        dh = d @ w
    return dgate


def lstmg_out_fwd(fc, bias, x, dtype=np.float64):
    """y (B, Co, T) = tanh(fc (B, T, out_ch) + bias + x (B, in_ch, T)) with torch's broadcast over the channel axis."""
    fc, bias, x = np.asarray(fc, dtype), np.asarray(bias, dtype), np.asarray(x, dtype)
    return np.tanh(fc.transpose(0, 2, 1) + bias[None, :, None] + x)


def lstmg_out_bwd(dy, y, out_ch, dtype=np.float64):
    """dpre (B, T, out_ch) = dy (1 - y^2) summed over the channels that broadcast onto each output channel."""
    dy, y = np.asarray(dy, dtype), np.asarray(y, dtype)
    d = dy * (dtype(1) - y * y)
    if out_ch != d.shape[1]:
        d = d.sum(1, keepdims=True, dtype=dtype)
    return d.transpose(0, 2, 1)


def gamma(n, u=2.0 ** -23):
    """n u / (1 - n u): the textbook bound of n roundings (inner products in any summation order)."""
    return n * u / (1.0 - n * u)

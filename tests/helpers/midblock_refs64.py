"""Independent references of the 64 -> 64 channel Spectral2DCNN blocks (blocks 2-6) on the f16x3 route, written from the ABI
text of include/modex_hip.h and the reference semantics it cites (LayerNorm -> Conv2d(64, 64, (5, 13), dilation (1, T), padding
same) -> + bias -> MaxPool2d((2, 1)), its data and weight gradients behind the pooling) with numpy only: no torch, no
autograd, no product code.  Everything computes in float64 unless said otherwise; tests/test_midblock_refs64.py holds each
function to torch's fp64 autograd and each layout to the convolution it must reproduce.

Layouts (the ABI's; PITCH = 352 positions per row, "+0 pad" = exact zeros at positions >= Wv):
* channels-last operand (B, H, 4, 352, 16): op[b][h][cb][w][j] = v[b][16 cb + j][h][w], +0 pad -- forward xhat, the routed
  gradient dz * S, and at pooled resolution (B, H / 2, ...) the pooled gradient G * S;
* dense weights (4, 5, 13, 2, 64, 8) = [cb][kh][kw][khalf][out][j] of W * 256, input channel 16 cb + 8 khalf + j;
  flip = 0: W[co = out][ci = in][kh][kw], flip = 1: W[co = in][ci = out][4 - kh][12 - kw];
* sparse data-gradient weights (4, 3, 2, 13, 2, 64, 16) = [cb][m][r][kwf][ci tile][lane][j] of W * 256: k = 16 (lane >> 5) + j,
  co = 16 cb + (k >> 1), kh = 4 + r - 2 m - (k & 1) (0 outside 0..4), kw = 12 - kwf, ci = 32 tile + (lane & 31);
* g_idx (B, H / 2, 4, 352) uint32: bits [16 hf + 2 j, + 2) = 2 (j & 1) + amax of channel 16 cb + (j < 4 ? 4 hf + j : 8 + 4 hf + j - 4);
* gidx (B, 64, H / 2, 22, 2) uint16: word (k-step ks, lane half hh), field j = 2 gq + e in bits [2 j, 2 j + 2) = 2 e + amax at
  position 16 ks + 8 (gq >> 1) + 4 hh + 2 (gq & 1) + e;
* f16x3 pair of a value v: hi = fp16(v), lo = fp16(v - hi).

u = 2^-23, gamma(n) = n u / (1 - n u): the rounding of n fp32 operations in any order.
"""
import functools

import numpy as np

from tests.helpers.block1_refs64 import (PITCH, ln_prelu_bwd, normalise, pack_pair, plane_stats, pool21, prelu,  # noqa: F401
                                         route, split16)

KH, KW, C = 5, 13, 64
TAPS = KH * KW
DILATIONS = (1, 2, 4, 8, 16)
WSCALE = 256.0
U = 2.0 ** -23
POISON = np.float32(1.0e30)
f16, f32, f64 = np.float16, np.float32, np.float64
W_ELEMS = 4 * KH * KW * 2 * C * 8
W_SP_ELEMS = 4 * 3 * 2 * KW * 2 * 64 * 16


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- the convolution and its two gradients ------------------------------------------------------------------------------
def _padded(v, T):
    v = np.asarray(v, f64)
    B, Cc, H, Wd = v.shape
    xp = np.zeros((B, Cc, H + KH - 1, Wd + (KW - 1) * T))
    xp[:, :, 2:2 + H, 6 * T:6 * T + Wd] = v
    return xp


def conv64(xhat, W, T):
    """z[b][co][h][w] = sum over (ci, kh, kw) of W[co][ci][kh][kw] xhat[b][ci][h + kh - 2][w + (kw - 6) T], zero outside the
    image (torch's Conv2d, dilation (1, T), padding "same", no bias): 65 shifted (co x ci) . (ci x B H W) products."""
    W = np.ascontiguousarray(np.asarray(W, f64).transpose(2, 3, 0, 1))     # [kh][kw][co][ci]: contiguous matrices
    B, Ci, H, Wd = np.shape(xhat)
    xp = _padded(xhat, T).transpose(1, 0, 2, 3)                             # channel first: one matrix product per tap
    z = np.zeros((W.shape[2], B * H * Wd))
    for kh in range(KH):
        for kw in range(KW):
            z += W[kh, kw] @ xp[:, :, kh:kh + H, kw * T:kw * T + Wd].reshape(Ci, B * H * Wd)
    return np.ascontiguousarray(z.reshape(W.shape[2], B, H, Wd).transpose(1, 0, 2, 3))


def conv64_pool_fwd(xhat, W, bias, T):
    """-> (out (B, 64, H / 2, W) = pooled z + bias, amax, z without the bias)."""
    z = conv64(xhat, W, T)
    pooled, amax = pool21(z)
    return pooled + np.asarray(bias, f64)[None, :, None, None], amax, z


def conv64_dgrad(dz, W, T):
    """dxhat[b][ci][h][w] = sum over (co, kh, kw) of dz[b][co][h - kh + 2][w - (kw - 6) T] W[co][ci][kh][kw]: every tap's
    (ci x co) . (co x B H W) product scattered to where the forward read it from."""
    W = np.ascontiguousarray(np.asarray(W, f64).transpose(2, 3, 1, 0))     # [kh][kw][ci][co]: contiguous matrices
    dz = np.asarray(dz, f64)
    B, Co, H, Wd = dz.shape
    dxp = np.zeros((W.shape[2], B, H + KH - 1, Wd + (KW - 1) * T))          # channel first: one matrix product per tap
    flat = dz.transpose(1, 0, 2, 3).reshape(Co, B * H * Wd)
    for kh in range(KH):
        for kw in range(KW):
            dxp[:, :, kh:kh + H, kw * T:kw * T + Wd] += (W[kh, kw] @ flat).reshape(-1, B, H, Wd)
    return np.ascontiguousarray(dxp[:, :, 2:2 + H, 6 * T:6 * T + Wd].transpose(1, 0, 2, 3))


def conv64_wgrad(dz, xhat, T):
    """dW[co][ci][kh][kw] = sum over (b, h, w) of dz[b][co][h][w] xhat[b][ci][h + kh - 2][w + (kw - 6) T]."""
    dz = np.asarray(dz, f64)
    B, Ci, H, Wd = np.shape(xhat)
    xp = _padded(xhat, T)
    dW = np.zeros((dz.shape[1], Ci, KH, KW))
    a = dz.transpose(1, 0, 2, 3).reshape(dz.shape[1], B * H * Wd)
    for kh in range(KH):
        for kw in range(KW):
            dW[:, :, kh, kw] = a @ xp[:, :, kh:kh + H, kw * T:kw * T + Wd].transpose(0, 2, 3, 1).reshape(B * H * Wd, Ci)
    return dW


def window_sum(v, T):
    """v (B, H, W) -> sum over the 65 taps of v[b][h + kh - 2][w + (kw - 6) T] (the window is symmetric: the same for the
    forward and the transposed convolution)."""
    xp = _padded(np.asarray(v, f64)[:, None], T)[:, 0]
    H, Wd = np.shape(v)[1:]
    return sum(xp[:, kh:kh + H, kw * T:kw * T + Wd] for kh in range(KH) for kw in range(KW))


def taps_inside(Wabs, H, Wd, T, transposed):
    """Wabs (n, 5, 13) = per output channel and tap the sum of |W| over the contracted channel -> (n, H, Wd): the sum over the
    taps that fall inside the image at (h, w) (forward: h + kh - 2, w + (kw - 6) T; transposed: h - kh + 2, w - (kw - 6) T)."""
    hh, ww = np.arange(H)[:, None], np.arange(Wd)[None, :]
    out = np.zeros((Wabs.shape[0], H, Wd))
    for kh in range(KH):
        for kw in range(KW):
            sh, sw = (kh - 2, (kw - 6) * T) if not transposed else (2 - kh, (6 - kw) * T)
            inside = ((hh + sh >= 0) & (hh + sh < H)) & ((ww + sw >= 0) & (ww + sw < Wd))
            out += Wabs[:, kh, kw, None, None] * inside
    return out


# ---- layouts --------------------------------------------------------------------------------------------------------------
def cl_layout(v, Wv):
    """v (B, 64, H, >= Wv) -> (B, H, 4, 352, 16) of v's dtype, +0 pad."""
    v = np.asarray(v)
    B, Cc, H = v.shape[:3]
    assert Cc == C
    out = np.zeros((B, H, 4, PITCH, 16), v.dtype)
    out[:, :, :, :Wv] = v[..., :Wv].reshape(B, 4, 16, H, Wv).transpose(0, 3, 1, 4, 2)
    return out


def cl_planes(op):
    """(B, H, 4, 352, 16) -> (B, 64, H, 352): the inverse of cl_layout on all 352 positions."""
    B, H = op.shape[:2]
    return op.transpose(0, 2, 4, 1, 3).reshape(B, C, H, PITCH)


def pack_weights(W, flip, scale=WSCALE):
    """W (64, 64, 5, 13) -> (4, 5, 13, 2, 64, 8) float64 of W * scale."""
    W = np.asarray(W, f64) * scale
    out = np.zeros((4, KH, KW, 2, C, 8))
    Wm = W[:, :, ::-1, ::-1]                                              # Wm[co][ci][kh'][kw'] = W[co][ci][4 - kh'][12 - kw']
    for cb in range(4):
        for khalf in range(2):
            cin = 16 * cb + 8 * khalf + np.arange(8)
            out[cb, :, :, khalf] = W[:, cin].transpose(2, 3, 0, 1) if not flip else Wm[cin].transpose(2, 3, 1, 0)
    return out


def pack_weights_sp(W, scale=WSCALE):
    """W (64, 64, 5, 13) -> (4, 3, 2, 13, 2, 64, 16) float64 of W * scale."""
    W = np.asarray(W, f64) * scale
    out = np.zeros((4, 3, 2, KW, 2, 64, 16))
    for cb in range(4):
        for m in range(3):
            for r in range(2):
                for k in range(32):
                    co, kh = 16 * cb + (k >> 1), 4 + r - 2 * m - (k & 1)
                    if 0 <= kh < KH:
                        s, j = k >> 4, k & 15
                        for tile in range(2):
                            out[cb, m, r, :, tile, 32 * s:32 * s + 32, j] = W[co, 32 * tile:32 * tile + 32, kh, ::-1].T
    return out


def _sp_channel(hf, j):
    return 4 * hf + j if j < 4 else 8 + 4 * hf + j - 4


def g_idx_words(amax):
    """amax (B, 64, H / 2, 352) -> (B, H / 2, 4, 352) uint32."""
    am = (np.asarray(amax).astype(np.uint32) & 1).reshape(amax.shape[0], 4, 16, amax.shape[2], PITCH)
    word = np.zeros((amax.shape[0], amax.shape[2], 4, PITCH), np.uint32)
    for hf in range(2):
        for j in range(8):
            f = np.uint32(2 * (j & 1)) + am[:, :, _sp_channel(hf, j)].transpose(0, 2, 1, 3)
            word |= f << np.uint32(16 * hf + 2 * j)
    return word


def gidx_words(amax):
    """amax (B, 64, H / 2, 352) -> (B, 64, H / 2, 22, 2) uint16."""
    am = np.asarray(amax).astype(np.uint16) & 1
    word = np.zeros(am.shape[:3] + (22, 2), np.uint16)
    for hh in range(2):
        for j in range(8):
            gq, e = j >> 1, j & 1
            pos = 16 * np.arange(22) + 8 * (gq >> 1) + 4 * hh + 2 * (gq & 1) + e
            word[..., hh] |= (np.uint16(2 * e) + am[..., pos]) << np.uint16(2 * j)
    return word


def routed_from_g_idx(g, g_idx):
    """What the sparse data gradient multiplies: g (B, Hp, 4, 352, 16) compressed values and their index words -> the logical
    operand (B, Hp, 4, 352, 32) with k = 2 (channel of the block) + row of the pair.  Element j of lane half hf lies in the
    group of four k = 4 (channel pair) .. + 3 at the place its 2-bit field names."""
    out = np.zeros(g.shape[:4] + (32,), g.dtype)
    for hf in range(2):
        for j in range(8):
            ch = _sp_channel(hf, j)
            field = (g_idx >> np.uint32(16 * hf + 2 * j)) & np.uint32(3)
            k = 4 * (ch >> 1) + field.astype(np.int64)
            np.put_along_axis(out, k[..., None], g[..., ch:ch + 1], axis=-1)
    return out


def routed_from_gidx(g, gidx):
    """What the sparse weight gradient multiplies: g (B, Hp, 4, 352, 16) and the planar words (B, 64, Hp, 22, 2) -> dz planes
    (B, 64, 2 Hp, 352).  Field j = 2 gq + e of (ks, hh) lies in the group of four k = 2 (position of the pair) + row at the
    place the field names; the pair of positions starts at 16 ks + 8 (gq >> 1) + 4 hh + 2 (gq & 1)."""
    gp = cl_planes(g)                                                    # (B, 64, Hp, 352)
    B, _, Hp, _ = gp.shape
    dz = np.zeros((B, C, 2 * Hp, PITCH), g.dtype)
    bi, ci, hi_ = np.meshgrid(np.arange(B), np.arange(C), np.arange(Hp), indexing="ij")
    for ks in range(22):
        for hh in range(2):
            for j in range(8):
                gq, e = j >> 1, j & 1
                base = 16 * ks + 8 * (gq >> 1) + 4 * hh + 2 * (gq & 1)
                field = ((gidx[:, :, :, ks, hh] >> np.uint16(2 * j)) & np.uint16(3)).astype(np.int64)
                dz[bi, ci, 2 * hi_ + (field & 1), base + (field >> 1)] = gp[:, :, :, base + e]
    return dz


# ---- the arithmetic the kernels are meant to do ---------------------------------------------------------------------------
DEFECTS = ("drop_hi_lo", "drop_lo_hi", "add_lo_lo", "halo_row", "halo_col", "last_tap_half_dilation", "taps_not_mirrored",
           "halves_swapped", "tie_to_odd_row", "argmax_bit_inverted", "last_slab_skipped", "scale_2s", "pad_351_nonzero")


def _acc32(a_hi, a_lo, b_hi, b_lo, order, defect):
    """(n, K) operand pairs -> (n,) float32: the products hi hi + hi lo + lo hi formed exactly (22-bit products of fp16
    numbers) and added to an fp32 accumulator one at a time, in the natural order (k ascending, the three products of a k
    together) or, "sorted", largest magnitude first (the small terms meet a large accumulator: the worst case)."""
    a_hi, a_lo, b_hi, b_lo = (np.asarray(v, f64) for v in (a_hi, a_lo, b_hi, b_lo))
    prods = [a_hi * b_hi]
    if defect != "drop_hi_lo":
        prods.append(a_hi * b_lo)
    if defect != "drop_lo_hi":
        prods.append(a_lo * b_hi)
    if defect == "add_lo_lo":
        prods.append(a_lo * b_lo)
    terms = np.stack(prods, -1).reshape(a_hi.shape[0], -1)
    if order == "sorted":
        terms = np.take_along_axis(terms, np.argsort(-np.abs(terms), axis=1, kind="stable"), axis=1)
    else:
        assert order == "natural"
    terms = terms[:, np.abs(terms).sum(0) > 0]                           # adding an exact zero rounds nothing
    t32 = terms.astype(f32)
    assert np.array_equal(t32.astype(f64), terms)                         # every product is an fp32 number
    acc = np.zeros(terms.shape[0], f32)
    for k in range(t32.shape[1]):
        acc = acc + t32[:, k]
    return acc


def _gather_conv(op, wpk, b, co, h, w, H, T, defect):
    """Operands of z[b][co][h][w] from a channels-last operand (B, H, 4, 352, 16) and dense packed weights: K = (cb, kh, kw,
    16 channels).  Rows outside the image are zero; positions outside 0..351 read the zero pad position 351."""
    n = len(b)
    cb, kh, kw, j = np.ix_(np.arange(4), np.arange(KH), np.arange(KW), np.arange(16))
    sh = lambda v: np.asarray(v)[:, None, None, None, None]
    rows = sh(h) + kh - 2 + 0 * (cb + kw + j)
    dil = np.where(kw == KW - 1, T // 2, T) if defect == "last_tap_half_dilation" else T
    cols = sh(w) + (kw - 6) * dil + 0 * (cb + kh + j)
    lo_r, lo_c = (-1 if defect == "halo_row" else 0), (-1 if defect == "halo_col" else 0)
    ok = (rows >= lo_r) & (rows < H)
    colz = np.where((cols >= lo_c) & (cols < PITCH), np.clip(cols, 0, PITCH - 1), PITCH - 1)
    a = op[sh(b), np.clip(rows, 0, H - 1), cb, colz, j] * ok
    bw = wpk[cb, kh, kw, j // 8, sh(co), j % 8] + 0 * rows
    return a.reshape(n, -1), bw.reshape(n, -1)


def f16x3_emulate(kind, ops, B, H, Wv, T, sel, order="natural", defect=None):
    """A numpy emulation of one f16x3 kernel on the operands the kernel itself is handed (``ops``: the documented layouts, as
    float16 / integer arrays), for the outputs ``sel`` names; CPU only.

    kind "fwd":      ops x_hi, x_lo, w_hi, w_lo (flip 0), bias;            sel (b, co, hp, w) -> (out float32, amax uint8)
    kind "dgrad":    ops dz_hi, dz_lo, w_hi, w_lo (flip 1), scale;          sel (b, ci, h, w)  -> dxhat float32
    kind "dgrad_sp": ops g_hi, g_lo, g_idx, w_hi, w_lo (sparse), scale;     sel (b, ci, h, w)  -> dxhat float32
    kind "wgrad":    ops dz_hi, dz_lo, x_hi, x_lo, scale, rows_per_slab;    sel (co, ci, kh, kw) -> dW float32
    kind "wgrad_sp": ops g_hi, g_lo, gidx, x_hi, x_lo, scale, rows_per_slab (pooled rows); sel (co, ci, kh, kw) -> dW float32
    scale = (S, 1 / S).  The weight gradients add each slab in fp32 and the slabs in fp64, like the kernels.
    ``defect``: one of DEFECTS, a deliberate deviation (tests/test_midblock_refs64.py::test_defects_are_seen)."""
    assert defect is None or defect in DEFECTS
    ops = dict(ops)
    sel = [np.asarray(s, np.int64) for s in sel]
    pair = lambda name: (np.array(ops[name + "_hi"], f64), np.array(ops[name + "_lo"], f64))
    inv_s = 1.0
    if "scale" in ops:
        inv_s = float(ops["scale"][1]) * (0.5 if defect == "scale_2s" else 1.0)
    first = {"fwd": "x", "dgrad": "dz", "dgrad_sp": "g", "wgrad": "x", "wgrad_sp": "x"}[kind]
    if defect == "pad_351_nonzero":                                       # the operand whose position 351 stands in for the halo
        for half, val in (("_hi", 8.0), ("_lo", 1.0)):
            a = np.array(ops[first + half], f64)
            a[:, :, :, PITCH - 1, :] = val
            ops[first + half] = a
    if kind in ("fwd", "dgrad"):
        w_hi, w_lo = (v.reshape(4, KH, KW, 2, C, 8) for v in pair("w"))
        if defect == "halves_swapped":
            w_hi, w_lo = w_hi[:, :, :, ::-1], w_lo[:, :, :, ::-1]
        if defect == "taps_not_mirrored" and kind == "dgrad":
            w_hi, w_lo = w_hi[:, ::-1, ::-1], w_lo[:, ::-1, ::-1]
        x_hi, x_lo = pair(first)
        if kind == "dgrad":
            b, ci, h, w = sel
            parts = [_gather_conv(x, wk, b, ci, h, w, H, T, defect) for x, wk in ((x_hi, w_hi), (x_lo, w_lo))]
            acc = _acc32(parts[0][0], parts[1][0], parts[0][1], parts[1][1], order, defect)
            return (acc.astype(f64) * (inv_s / WSCALE)).astype(f32)
        b, co, hp, w = sel
        rows = []
        for r in range(2):
            parts = [_gather_conv(x, wk, b, co, 2 * hp + r, w, H, T, defect) for x, wk in ((x_hi, w_hi), (x_lo, w_lo))]
            rows.append(_acc32(parts[0][0], parts[1][0], parts[0][1], parts[1][1], order, defect))
        take = rows[1] >= rows[0] if defect == "tie_to_odd_row" else rows[1] > rows[0]
        v = np.where(take, rows[1], rows[0]) * f32(1.0 / WSCALE) + np.asarray(ops["bias"], f32)[co]
        return v.astype(f32), take.astype(np.uint8)
    if kind == "dgrad_sp":
        g_idx = np.array(ops["g_idx"], np.uint32)
        if defect == "argmax_bit_inverted":
            g_idx = g_idx ^ np.uint32(1)                                    # field 0 of lane half 0: channel 16 cb
        r_hi, r_lo = (routed_from_g_idx(g, g_idx) for g in pair("g"))
        w_hi, w_lo = (v.reshape(4, 3, 2, KW, 2, 64, 16) for v in pair("w"))
        if defect == "halves_swapped":                                     # the two k halves of a fragment
            w_hi, w_lo = (np.concatenate([v[..., 32:, :], v[..., :32, :]], -2) for v in (w_hi, w_lo))
        if defect == "taps_not_mirrored":
            w_hi, w_lo = w_hi[:, :, :, ::-1], w_lo[:, :, :, ::-1]
        b, ci, h, w = sel
        n, Hp = len(b), H // 2
        cb, m, kwf, k = np.ix_(np.arange(4), np.arange(3), np.arange(KW), np.arange(32))
        sh = lambda v: np.asarray(v)[:, None, None, None, None]
        prow = sh(h // 2) + m - 1 + 0 * (cb + kwf + k)
        dil = np.where(kwf == KW - 1, T // 2, T) if defect == "last_tap_half_dilation" else T
        cols = sh(w) + (kwf - 6) * dil + 0 * (cb + m + k)
        lo_r, lo_c = (-1 if defect == "halo_row" else 0), (-1 if defect == "halo_col" else 0)
        ok = (prow >= lo_r) & (prow < Hp)
        colz = np.where((cols >= lo_c) & (cols < PITCH), np.clip(cols, 0, PITCH - 1), PITCH - 1)
        ga = lambda r_: (r_[sh(b), np.clip(prow, 0, Hp - 1), cb, colz, k] * ok).reshape(n, -1)
        gw = lambda w_: (w_[cb, m, sh(h % 2), kwf, sh(ci // 32), sh(ci % 32) + 32 * (k // 16), k % 16] + 0 * prow).reshape(n, -1)
        acc = _acc32(ga(r_hi), ga(r_lo), gw(w_hi), gw(w_lo), order, defect)
        return (acc.astype(f64) * (inv_s / WSCALE)).astype(f32)
    # ---- weight gradients: K = the positions of a slab
    if kind == "wgrad":
        dz_hi, dz_lo = (cl_planes(v) for v in pair("dz"))
        slab_rows = int(ops["rows_per_slab"])
    else:
        gidx = np.array(ops["gidx"], np.uint16)
        if defect == "argmax_bit_inverted":
            gidx = gidx ^ np.uint16(1)                                      # field 0 of every word: positions 16 ks + 4 hh
        dz_hi, dz_lo = (routed_from_gidx(g, gidx) for g in pair("g"))
        slab_rows = 2 * int(ops["rows_per_slab"])
    x_hi, x_lo = (cl_planes(v) for v in pair("x"))
    co, ci, kh, kw = sel
    ci_x = ci ^ 8 if defect == "halves_swapped" else ci                   # the other 8-channel half of the x operand's block
    n, n_rows = len(co), B * H
    n_slabs = -(-n_rows // slab_rows)
    total = np.zeros(n)
    for slab in range(n_slabs - (1 if defect == "last_slab_skipped" else 0)):
        rid = np.arange(slab * slab_rows, min((slab + 1) * slab_rows, n_rows))
        bb, hh = (rid // H)[:, None], (rid % H)[:, None]
        ww = np.arange(PITCH)[None, :]
        sh = lambda v: np.asarray(v)[:, None, None]
        rows = hh[None] + sh(kh) - 2 + 0 * ww[None]
        dil = np.where(sh(kw) == KW - 1, T // 2, T) if defect == "last_tap_half_dilation" else T
        cols = ww[None] + (sh(kw) - 6) * dil + 0 * hh[None]
        lo_r, lo_c = (-1 if defect == "halo_row" else 0), (-1 if defect == "halo_col" else 0)
        ok = (rows >= lo_r) & (rows < H)
        colz = np.where((cols >= lo_c) & (cols < PITCH), np.clip(cols, 0, PITCH - 1), PITCH - 1)
        gx = lambda x_: (x_[bb[None], sh(ci_x), np.clip(rows, 0, H - 1), colz] * ok).reshape(n, -1)
        gd = lambda d_: (d_[bb[None], sh(co), hh[None], ww[None]] + 0 * rows).reshape(n, -1)
        total += _acc32(gd(dz_hi), gd(dz_lo), gx(x_hi), gx(x_lo), order, defect).astype(f64)
    return (total * inv_s).astype(f32)


# ---- problems shared by the CPU and the GPU tests -------------------------------------------------------------------------
def _freeze(pr):
    for a in pr.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return pr


def _i16(a):
    a16 = np.asarray(a).astype(f16)
    assert np.array_equal(a16.astype(f64), a)
    return a16


@functools.lru_cache(maxsize=None)
def exact_inputs(B, H, Wv):
    """Integer operands: hi = 8 a, lo = b with |a|, |b| <= 3, so that a term hi hi + hi lo + lo hi is at most 24 * 24 + 2 * 24 * 3 = 720
    and every partial sum over the 4160 taps (or the B * H / 2 * Wv routed positions) an integer below 2^24 (asserted where the
    sums are formed); bias a multiple of 1 / 256; S = 4.  The last clip (B > 1) has all rows alike: interior pooling pairs tie."""
    g = np.random.default_rng(B * 10000 + H * 1000 + Wv)
    Hp = H // 2
    ints = lambda *shape: g.integers(-3, 4, shape).astype(f64)
    xh, xl = 8.0 * ints(B, C, H, Wv), ints(B, C, H, Wv)
    if B > 1:
        xh[B - 1], xl[B - 1] = xh[B - 1, :, :1], xl[B - 1, :, :1]
    gh, gl = 8.0 * ints(B, C, Hp, Wv), ints(B, C, Hp, Wv)
    amax = g.integers(0, 2, (B, C, Hp, PITCH)).astype(np.uint8)             # the pad positions too: they have index words
    bias = g.integers(-1024, 1025, C) / 256.0
    return _freeze(dict(xh=xh, xl=xl, gh=gh, gl=gl, amax=amax, bias=bias, S=4.0,
                        x_hi=_i16(cl_layout(xh, Wv)), x_lo=_i16(cl_layout(xl, Wv)), scale=np.array([4.0, 0.25], f32)))


@functools.lru_cache(maxsize=None)
def exact_weights():
    """The weight operands of exact_inputs in all three packings (the same W for every shape)."""
    g = np.random.default_rng(64)
    wh, wl = 8.0 * g.integers(-3, 4, (C, C, KH, KW)), g.integers(-3, 4, (C, C, KH, KW)).astype(f64)
    pr = dict(wh=wh, wl=wl)
    for name, fn in (("fwd", lambda w: pack_weights(w, 0, 1.0)), ("flip", lambda w: pack_weights(w, 1, 1.0)),
                     ("sp", lambda w: pack_weights_sp(w, 1.0))):
        pr[name + "_hi"], pr[name + "_lo"] = _i16(fn(wh)), _i16(fn(wl))
    return _freeze(pr)


@functools.lru_cache(maxsize=None)
def exact_fwd(B, H, Wv, T):
    i, w = exact_inputs(B, H, Wv), exact_weights()
    wh, wl = w["wh"], w["wl"]
    worst = ((np.abs(wh) + np.abs(wl)).sum((1, 2, 3)) * np.abs(i["xh"]).max() + np.abs(wh).sum((1, 2, 3)) * np.abs(i["xl"]).max()
             + 256 * np.abs(i["bias"]))
    assert worst.max() < 2.0 ** 24
    acc = conv64(i["xh"], wh + wl, T) + conv64(i["xl"], wh, T)              # hi hi + hi lo + lo hi; lo lo is dropped by design
    pooled, amax = pool21(acc)
    out = pooled / 256.0 + i["bias"][None, :, None, None]
    assert np.array_equal(out, out.astype(f32).astype(f64))
    return _freeze(dict(out=out.astype(f32), amax=amax, ties=int((acc[:, :, 1::2] == acc[:, :, 0::2]).sum())))


@functools.lru_cache(maxsize=None)
def exact_grad_operands(B, H, Wv):
    i = exact_inputs(B, H, Wv)
    av = i["amax"][..., :Wv]
    dzh, dzl = route(i["gh"], av), route(i["gl"], av)
    return _freeze(dict(dzh=dzh, dzl=dzl, dz_hi=_i16(cl_layout(dzh, Wv)), dz_lo=_i16(cl_layout(dzl, Wv)),
                        g_hi=_i16(cl_layout(i["gh"], Wv)), g_lo=_i16(cl_layout(i["gl"], Wv)),
                        g_idx=g_idx_words(i["amax"]), gidx=gidx_words(i["amax"])))


@functools.lru_cache(maxsize=None)
def exact_dgrad(B, H, Wv, T):
    i, w, o = exact_inputs(B, H, Wv), exact_weights(), exact_grad_operands(B, H, Wv)
    wh, wl = w["wh"], w["wl"]
    worst = (np.abs(wh) + np.abs(wl)).sum((0, 2, 3)) * np.abs(o["dzh"]).max() + np.abs(wh).sum((0, 2, 3)) * np.abs(o["dzl"]).max()
    assert worst.max() < 2.0 ** 24
    dx = (conv64_dgrad(o["dzh"], wh + wl, T) + conv64_dgrad(o["dzl"], wh, T)) / (256.0 * i["S"])
    assert np.array_equal(dx, dx.astype(f32).astype(f64))
    return _freeze(dict(dx=dx.astype(f32)))


@functools.lru_cache(maxsize=None)
def exact_wgrad(B, H, Wv, T):
    i, o = exact_inputs(B, H, Wv), exact_grad_operands(B, H, Wv)
    # one routed position per pooling pair: B * H / 2 * Wv terms of at most 720
    assert B * (H // 2) * Wv * (np.abs(o["dzh"]).max() * (np.abs(i["xh"]).max() + np.abs(i["xl"]).max())
                                + np.abs(o["dzl"]).max() * np.abs(i["xh"]).max()) < 2.0 ** 24
    dW = (conv64_wgrad(o["dzh"], i["xh"] + i["xl"], T) + conv64_wgrad(o["dzl"], i["xh"], T)) / i["S"]
    assert np.array_equal(dW, dW.astype(f32).astype(f64))
    return _freeze(dict(dW=dW.astype(f32)))


# (B, H, Wv) of the GPU tests.  B * H / 2 a multiple of 8 (the kernels renumber their workgroups): (2, 8, 345), (1, 16, 1),
# (2, 16, 88); H = 2: every halo row outside; Wv = 1, 17, 40: taps outside on both sides; 351: the widest the sparse kernels take
EXACT_SHAPES = ((1, 2, 17), (2, 8, 345), (3, 6, 40), (2, 4, 351), (1, 16, 1), (2, 16, 88))
EXACT_SHAPES_DENSE = EXACT_SHAPES + ((2, 4, 352),)
ROUNDING_SHAPES = ((2, 4, 345), (3, 6, 40))


def pow2_scale(m):
    """The power of two S with m S in [512, 1024)."""
    return 2.0 ** (10 - int(np.frexp(f32(m))[1]))


def heavy_tailed(g, shape):
    """Magnitudes 2^-k, k uniform in 0..14, random signs, a handful at full scale."""
    v = (2.0 ** -g.integers(0, 15, shape).astype(f64)) * g.choice([-1.0, 1.0], shape)
    flat = v.reshape(-1)
    flat[g.integers(0, flat.size, 5)] = 1.0
    return v.astype(f32)


@functools.lru_cache(maxsize=None)
def float_inputs(B, H, Wv, kind="gauss"):
    """Random fp32 inputs of one block: x = the previous block's pooled pre-activations (B, 64, H, 352), the PReLU slope in
    front, the statistics of PReLU(x) in fp32, W, bias, the pooled gradient G (B, 64, H / 2, 352) (Gaussian or heavy-tailed)
    and a random argmax; the pad positions of x and G hold 1e30."""
    g = np.random.default_rng(B * 10000 + H * 1000 + Wv)                    # x, W, bias: the same for both kinds of G
    gg = np.random.default_rng(B * 10000 + H * 1000 + Wv + (7 if kind == "heavy" else 3))
    Hp = H // 2
    x = np.full((B, C, H, PITCH), POISON, f32)
    x[..., :Wv] = (g.standard_normal((B, C, H, Wv)) * 0.7 + 0.1).astype(f32)
    slope = g.uniform(0.05, 0.45, C).astype(f32)
    stats = plane_stats(prelu(x[..., :Wv].astype(f64), slope.astype(f64)[None, :, None, None])).astype(f32)
    W = (g.standard_normal((C, C, KH, KW)) / np.sqrt(C * TAPS)).astype(f32)
    bias = (g.standard_normal(C) * 0.1).astype(f32)
    G = np.full((B, C, Hp, PITCH), POISON, f32)
    G[..., :Wv] = heavy_tailed(gg, (B, C, Hp, Wv)) if kind == "heavy" else (gg.standard_normal((B, C, Hp, Wv)) * 1e-3).astype(f32)
    amax = gg.integers(0, 2, (B, C, Hp, PITCH)).astype(np.uint8)
    y = prelu(x[..., :Wv].astype(f64), slope.astype(f64)[None, :, None, None])
    m, r = stats.astype(f64)[:, :, 0, None, None], stats.astype(f64)[:, :, 1, None, None]
    return _freeze(dict(x=x, slope=slope, stats=stats, W=W, bias=bias, G=G, amax=amax, xhat=(y - m) * r,
                        xhat_mag=(np.abs(y) + np.abs(m)) * r, dz=route(G[..., :Wv], amax[..., :Wv])))


@functools.lru_cache(maxsize=None)
def host_operands(B, H, Wv, kind="gauss", shift=0):
    """The operands the device preparation kernels make from float_inputs, made here with the same fp32 operations (CPU
    emulation only): the forward pair, the pooled and the routed gradient pairs on S = pow2_scale(max |G|) / 2^shift."""
    i = float_inputs(B, H, Wv, kind)
    xv, sl = i["x"][..., :Wv], i["slope"][None, :, None, None]
    t = np.where(xv > 0, xv, sl * xv).astype(f32)
    xh32 = ((t - i["stats"][:, :, 0, None, None]).astype(f32) * i["stats"][:, :, 1, None, None]).astype(f32)
    S = pow2_scale(np.abs(i["G"][..., :Wv]).max()) / 2.0 ** shift
    gs = (i["G"][..., :Wv].astype(f64) * S).astype(f32)
    ops = dict(scale=np.array([S, 1.0 / S], f32), g_idx=g_idx_words(i["amax"]), gidx=gidx_words(i["amax"]))
    for name, v in (("x", xh32), ("g", gs), ("dz", route(gs, i["amax"][..., :Wv]).astype(f32))):
        ops[name + "_hi"], ops[name + "_lo"] = (cl_layout(h, Wv) for h in split16(v))
    return _freeze(dict(ops, **_host_weights(B, H, Wv)))


@functools.lru_cache(maxsize=None)
def _host_weights(B, H, Wv):
    W = float_inputs(B, H, Wv)["W"]                                           # (the same W for both kinds of gradient)
    ops = {}
    for name, wp in (("wf", pack_weights(W, 0)), ("wflip", pack_weights(W, 1)), ("wsp", pack_weights_sp(W))):
        ops[name + "_hi"], ops[name + "_lo"] = split16(wp)
    return ops


# ---- per-element bounds of the float problems ------------------------------------------------------------------------------
# A pair represents its value v to 2^-22 |v| + 2^-25 (block1_refs64); the product of two pairs without lo lo then differs from
# the product of the values by 3 x 2^-22 of its magnitude (two representations + the dropped term) plus 2^-25 (1 + 2^-10) of the
# OTHER operand (the absolute part of each representation; 2^-10: its share in lo lo).  n fp32 additions in any order and the
# two final operations (the scale product, the bias or the fp64 -> fp32 rounding): gamma(n + 2) of the sum of magnitudes.
REL = 3 * 2.0 ** -22
ABS = 2.0 ** -25 * (1 + 2.0 ** -10)
N_CONV = 3 * C * TAPS                                                       # 12480 accumulated products per output


@functools.lru_cache(maxsize=None)
def float_fwd(B, H, Wv, T):
    """-> out, amax, z, and per element of z the bound; the forward operand is made with 3 fp32 operations (slope product,
    - mean, * rstd: 3 u of xhat_mag), the weight operand with none."""
    i = float_inputs(B, H, Wv)
    W64 = i["W"].astype(f64)
    out, amax, z = conv64_pool_fwd(i["xhat"], W64, i["bias"], T)
    mag = conv64(i["xhat_mag"], np.abs(W64), T)
    absw = taps_inside(np.abs(W64).sum(1), H, Wv, T, False)[None]            # error 2^-25 of each xhat operand x |W * 256| / 256
    absx = window_sum(np.abs(i["xhat"]).sum(1), T)[:, None] / WSCALE         # error 2^-25 of each W * 256 operand x |xhat| / 256
    zb = (REL + 3 * U + gamma(N_CONV + 2)) * mag + ABS * (absw + absx)
    return _freeze(dict(out=out, amax=amax, z=z, zbound=zb))


@functools.lru_cache(maxsize=None)
def _float_dgrad_core(B, H, Wv, T, kind):
    i = float_inputs(B, H, Wv, kind)
    W64, dz = i["W"].astype(f64), i["dz"]
    return _freeze(dict(dx=conv64_dgrad(dz, W64, T), mag=conv64_dgrad(np.abs(dz), np.abs(W64), T),
                        absw=taps_inside(np.abs(W64).sum(0), H, Wv, T, True)[None],
                        absg=window_sum(np.abs(dz).sum(1), T)[:, None] / WSCALE))


def float_dgrad(B, H, Wv, T, kind, shift):
    """-> dxhat and its bound on the scale S = pow2_scale(max |G|) / 2^shift: G * S is exact, its pair is within
    2^-22 |G S| + 2^-25, i.e. 2^-25 / S after the scaling back (times |W * 256| / 256 over the taps inside the image); the
    W * 256 pair's 2^-25 meets |dz| / 256."""
    c = _float_dgrad_core(B, H, Wv, T, kind)
    S = pow2_scale(np.abs(float_inputs(B, H, Wv, kind)["G"][..., :Wv]).max()) / 2.0 ** shift
    return dict(dx=c["dx"], bound=(REL + gamma(N_CONV + 2)) * c["mag"] + ABS * (c["absw"] / S + c["absg"]), S=S)


@functools.lru_cache(maxsize=None)
def _float_wgrad_core(B, H, Wv, T, kind):
    i = float_inputs(B, H, Wv, kind)
    return _freeze(dict(dW=conv64_wgrad(i["dz"], i["xhat"], T), mag=conv64_wgrad(np.abs(i["dz"]), i["xhat_mag"], T)))


def float_wgrad(B, H, Wv, T, kind, shift):
    """-> dW and the parts of its bound: ``mag`` = sum |dz| xhat_mag and ``abs`` = the absolute parts of the two pairs over all
    positions (an upper bound: 2^-25 / S on every xhat of the plane, 2^-25 on every dz).  The bound of a run with r rows of
    Wv positions per slab is wgrad_bound(pr, 3 * r * Wv)."""
    i, c = float_inputs(B, H, Wv, kind), _float_wgrad_core(B, H, Wv, T, kind)
    S = pow2_scale(np.abs(i["G"][..., :Wv]).max()) / 2.0 ** shift
    ab = ABS * (np.abs(i["xhat"]).sum((0, 2, 3))[None, :, None, None] / S + np.abs(i["dz"]).sum((0, 2, 3))[:, None, None, None])
    return dict(dW=c["dW"], mag=c["mag"], abs=ab, S=S)


def wgrad_bound(pr, n_products):
    """3 x 2^-22 + 3 u (the forward operand's own operations) + gamma(products of a slab + 2): the slabs add in fp64, the
    product with 1 / S and the rounding to fp32 are the 2."""
    return (REL + 3 * U + gamma(n_products + 2)) * pr["mag"] + pr["abs"]

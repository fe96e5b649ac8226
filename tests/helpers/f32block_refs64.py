"""References, problems, bounds and an fp32 emulation for the exact-fp32 conv block kernels (K5/K6: mx_conv_pack_weights,
mx_plane_stats, mx_plane_sum, mx_conv_block_fwd, mx_conv_block_dgrad, mx_conv_block_wgrad), written from the ABI text of
include/modex_hip.h with numpy only: no torch, no product code.  The convolution and its two gradients are
midblock_refs64.conv64 / conv64_dgrad / conv64_wgrad (generic in the channel count), the statistics, PReLU, pooling and routing
are block1_refs64's; tests/test_f32block_refs64.py holds them to torch's fp64 autograd at Cin = 2 with a dilation.

Layouts (the ABI's; PITCH = 352 floats per row, Wv valid columns):
* activation planes (B, C, H, 352) fp32; the kernels must not let a column >= Wv of an input reach a result;
* packed weights of W (Cout, Cin, 5, 13): flip = 0 -> [ci][kh][kw][co], flip = 1 -> [co][4 - kh][12 - kw][ci];
* the weight gradient's workspace ``part`` (slab, kh, kw, co, ci): slab s holds the sum over the rows
  s * rows_per_slab .. of the B * H rows (b, h) taken in order; dW is their fp64 sum over the slabs rounded once.

Exact problems.  x holds integers |x| <= 3, the statistics are GIVEN with an integer mean |m| <= 2 and rstd in {1/2, 1, 2},
slopes are in {1/4, 1/2, 1}: PReLU(x) is a multiple of 1/4 and xhat = (PReLU(x) - m) rstd a multiple of the quantum q = 1/8 with
|xhat| <= 10 = 80 q.  W, bias and G are integers of magnitude <= 3.  Every product and every partial sum of a convolution
output is then a multiple of q (dgrad: of 1), and the sums of magnitudes stay below 2^24 q (asserted from the fp64 sums of
magnitudes where the references are formed): every fp32 operation of the kernels -- the slope product, the subtraction, the
scale, the fused multiply-adds of the matrix instruction in ANY order, the bias add, the per-slab partials -- is exact, the fp64
sum over the slabs is exact, and the results must equal the fp64 reference bit for bit.  Ties between the two pooled rows are
frequent by construction (exact_problem), which pins "first max on ties".

Float problems and their two gates (tests/test_gpu_f32block_units.py applies both as ratio <= 1).  The reference is the fp64
evaluation of the same fp32 inputs WITH THE GIVEN fp32 STATISTICS (statistics are inputs of these kernels).
u = 2^-23, gamma(n) = n u / (1 - n u): n fp32 roundings in any order (u is twice the unit roundoff of round-to-nearest, which
covers the second-order terms dropped below).

Gate A, per element.  xhat = ((PReLU(x)) - mean) rstd carries at most three fp32 roundings (slope product, subtraction, scale),
each relative to an intermediate of magnitude <= rstd (|PReLU(x)| + |mean|) =: xhat_mag, so e_x <= gamma(3) xhat_mag.  A
convolution output is the sum of n = 65 Cin (forward), 65 * 64 (data gradient) products accumulated in fp32 by fused
multiply-adds: |err| <= gamma(n + 1) sum |w| |xhat| + sum |w| e_x, both sums formed by the reference convolution of the
magnitudes (the data gradient's operand, the routed G, is exact: no second term).  max(a, b) moves by at most the larger of the
two rows' errors, and the bias add is one more rounding: the pooled output's bound is max(row bounds) + u |out|.  The weight
gradient sums n = B H Wv products (fp32 inside a slab, fp64 across the slabs: at most n fp32 additions in all), then one fp32
addition that joins the two halves of a slab's partial and the final conversion: (gamma(n + 1) + 2 u) sum |dz| |xhat| +
sum |dz| e_x.

Gate B, the project's parity numbers against fp64: worst error over the tensor's maximum <= 5e-6 (forward), <= 1e-5 (dxhat and
dW).  Gate A is a worst-case bound (about 5e-3 of max |z| at Cin = 64); Gate B is what notices operands truncated to a
reduced-precision matrix type.

Pooling decisions of the float problems: the argmax must equal the reference's wherever the fp64 gap |z1 - z0| exceeds
BAND * max |z|, BAND = 1e-5 (Gate B's scale: twice the forward's gate on each row); inside the band either row is accepted, and
the share of elements inside it is at most BAND_SHARE = 1e-3 (asserted from the reference alone: float_fwd).
"""
import functools

import numpy as np

from tests.helpers import midblock_refs64 as M
from tests.helpers.block1_refs64 import PITCH, normalise, plane_stats, pool21, prelu, route  # noqa: F401
from tests.helpers.midblock_refs64 import (DILATIONS, EXACT_SHAPES_DENSE, ROUNDING_SHAPES, conv64, conv64_dgrad,  # noqa: F401
                                           conv64_wgrad, gamma, heavy_tailed)

KH, KW, CO = 5, 13, 64
TAPS = KH * KW
U = 2.0 ** -23
POISON = np.float32(1.0e30)
f32, f64 = np.float32, np.float64
GATE_B = {"fwd": 5e-6, "dgrad": 1e-5, "wgrad": 1e-5}
BAND, BAND_SHARE = 1e-5, 1e-3
QUANTUM = 0.125

DEFECTS = ("tie_takes_second", "halo_row", "halo_col", "last_tap_half_dilation", "taps_not_mirrored", "pad_leaks",
           "stats_of_clip_0", "slab_last_row_dropped", "prelu_skipped", "route_ignores_amax", "operands_truncated_to_tf32")


def _freeze(pr):
    for a in pr.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return pr


# ---- layouts ----------------------------------------------------------------------------------------------------------------
def pack_weights(W, flip):
    """W (Cout, Cin, 5, 13) -> flip 0: (Cin, 5, 13, Cout) = [ci][kh][kw][co]; flip 1: (Cout, 5, 13, Cin) = [co][4 - kh][12 - kw][ci]."""
    W = np.asarray(W)
    if not flip:
        return np.ascontiguousarray(W.transpose(1, 2, 3, 0))
    return np.ascontiguousarray(W[:, :, ::-1, ::-1].transpose(0, 2, 3, 1))


def part_layout(dW_slabs):
    """Per-slab weight gradients (S, 64, Cin, 5, 13) -> the workspace's (S, 5, 13, 64, Cin)."""
    return np.ascontiguousarray(np.asarray(dW_slabs).transpose(0, 3, 4, 1, 2))


def slab_rows(B, H, rows_per_slab):
    """The row ids (b * H + h) of every slab."""
    n = B * H
    return [np.arange(s, min(s + rows_per_slab, n)) for s in range(0, n, rows_per_slab)]


def wgrad_parts(dz, xhat, T, B, H, rows_per_slab):
    """-> (S, 64, Cin, 5, 13): the weight gradient of every slab's rows alone (fp64)."""
    dz = np.asarray(dz, f64)
    out = []
    for rid in slab_rows(B, H, rows_per_slab):
        d = np.zeros_like(dz)
        d[rid // H, :, rid % H] = dz[rid // H, :, rid % H]
        out.append(conv64_wgrad(d, xhat, T))
    return np.stack(out)


def planes(v, Wv, fill=POISON, dtype=f32):
    """v (..., Wv) -> (..., 352) with ``fill`` in the pad columns."""
    v = np.asarray(v)
    out = np.full(v.shape[:-1] + (PITCH,), fill, dtype)
    out[..., :Wv] = v
    return out


def poisoned_amax(g, amax, Wv):
    """amax (..., Wv) in {0, 1} -> (..., 352) uint8 with 0 / 1 / 2 mixed in the pad columns."""
    out = g.integers(0, 3, amax.shape[:-1] + (PITCH,)).astype(np.uint8)
    out[..., :Wv] = amax
    return out


# ---- exact problems ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_problem(B, H, Wv, Cin):
    """Integer inputs of one block with Cin input channels (Cin = 2: the first layer, no slope).  Ties: the rows of the last
    clip (B > 1; of the only clip from row 4 on, or all of them at H = 2) are alike, so its interior pooling pairs tie; the
    output channels co % 16 == 0 have weights symmetric in kh with zero rows kh = 1, 3, so that on such a clip the pairs at the
    image's edge tie as well (H = 2, 4)."""
    g = np.random.default_rng(B * 10000 + H * 1000 + Wv + 7 * Cin)
    Hp = H // 2
    ints = lambda lo, hi, *shape: g.integers(lo, hi + 1, shape).astype(f64)
    x = ints(-3, 3, B, Cin, H, Wv)
    if B > 1 or H == 2:
        x[B - 1] = x[B - 1, :, :1]
    elif H > 8:
        x[0, :, 4:] = x[0, :, 4:5]
    mean = ints(-2, 2, B, Cin)
    rstd = g.choice([0.5, 1.0, 2.0], (B, Cin))
    slope = None if Cin == 2 else g.choice([0.25, 0.5, 1.0], Cin)
    W = ints(-3, 3, CO, Cin, KH, KW)
    W[::16, :, 3], W[::16, :, 4] = 0.0, W[::16, :, 0]
    W[::16, :, 1] = 0.0
    bias = ints(-3, 3, CO)
    G = ints(-3, 3, B, CO, Hp, Wv)
    amax = g.integers(0, 2, (B, CO, Hp, Wv)).astype(np.uint8)
    y = x if slope is None else prelu(x, slope[None, :, None, None])
    stats = np.stack([mean, rstd], -1)
    xhat = normalise(y, stats)
    assert np.array_equal(xhat / QUANTUM, np.round(xhat / QUANTUM)) and np.abs(xhat).max() <= 10
    return _freeze(dict(x=planes(x, Wv), stats=stats.astype(f32), slope=None if slope is None else slope.astype(f32), W=W.astype(f32),
                        bias=bias.astype(f32), G=planes(G, Wv), amax=poisoned_amax(g, amax, Wv), xhat=xhat,
                        dz=route(G, amax)))


def _f32_exact(v):
    v = np.asarray(v, f64) + 0.0                                              # (-0 -> +0: an fp32 sum from +0 never gives -0)
    assert np.array_equal(v, v.astype(f32).astype(f64))
    return v.astype(f32)


@functools.lru_cache(maxsize=None)
def exact_fwd(B, H, Wv, Cin, T):
    p = exact_problem(B, H, Wv, Cin)
    W = p["W"].astype(f64)
    worst = conv64(np.abs(p["xhat"]), np.abs(W), T).max() + np.abs(p["bias"]).max()
    assert worst / QUANTUM < 2.0 ** 24
    z = conv64(p["xhat"], W, T)
    pooled, amax = pool21(z)
    return _freeze(dict(out=_f32_exact(pooled + p["bias"].astype(f64)[None, :, None, None]), amax=amax,
                        ties=int((z[:, :, 1::2] == z[:, :, 0::2]).sum())))


@functools.lru_cache(maxsize=None)
def exact_dgrad(B, H, Wv, T):
    p = exact_problem(B, H, Wv, 64)
    W = p["W"].astype(f64)
    assert conv64_dgrad(np.abs(p["dz"]), np.abs(W), T).max() < 2.0 ** 24
    return _freeze(dict(dx=_f32_exact(conv64_dgrad(p["dz"], W, T))))


@functools.lru_cache(maxsize=None)
def exact_wgrad(B, H, Wv, Cin, T):
    p = exact_problem(B, H, Wv, Cin)
    assert conv64_wgrad(np.abs(p["dz"]), np.abs(p["xhat"]), T).max() / QUANTUM < 2.0 ** 24
    return _freeze(dict(dW=_f32_exact(conv64_wgrad(p["dz"], p["xhat"], T))))


@functools.lru_cache(maxsize=None)
def exact_wgrad_parts(B, H, Wv, Cin, T, rows_per_slab):
    """The workspace (slab, kh, kw, co, ci) of the exact problem: every slab's partial is exact as well (its sum of magnitudes
    is part of the whole's)."""
    p = exact_problem(B, H, Wv, Cin)
    exact_wgrad(B, H, Wv, Cin, T)                                              # (the magnitude assertion)
    parts = _f32_exact(part_layout(wgrad_parts(p["dz"], p["xhat"], T, B, H, rows_per_slab)))
    parts.setflags(write=False)
    return parts


# ---- float problems ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def float_problem(B, H, Wv, Cin):
    """x = 0.7 N(0, 1) + 0.1, W = N(0, 1) / sqrt(65 Cin), the statistics of PReLU(x) (Cin = 2: of x) rounded to fp32 and then
    GIVEN; Cin = 64: midblock_refs64.float_inputs' tensors."""
    if Cin == 64:
        i = M.float_inputs(B, H, Wv)
        x, slope, stats, W, bias = (i[k] for k in ("x", "slope", "stats", "W", "bias"))
    else:
        g = np.random.default_rng(B * 10000 + H * 1000 + Wv + 13 * Cin)
        x = planes((g.standard_normal((B, Cin, H, Wv)) * 0.7 + 0.1).astype(f32), Wv)
        slope = None if Cin == 2 else g.uniform(0.05, 0.45, Cin).astype(f32)
        W = (g.standard_normal((CO, Cin, KH, KW)) / np.sqrt(Cin * TAPS)).astype(f32)
        bias = (g.standard_normal(CO) * 0.1).astype(f32)
        xv = x[..., :Wv].astype(f64)
        stats = plane_stats(xv if slope is None else prelu(xv, slope.astype(f64)[None, :, None, None])).astype(f32)
    xv = x[..., :Wv].astype(f64)
    y = xv if slope is None else prelu(xv, slope.astype(f64)[None, :, None, None])
    m, r = stats.astype(f64)[:, :, 0, None, None], stats.astype(f64)[:, :, 1, None, None]
    return _freeze(dict(x=x, slope=slope, stats=stats, W=W, bias=bias, xhat=(y - m) * r, xhat_mag=(np.abs(y) + np.abs(m)) * r))


GRAD_KINDS = ("gauss", "heavy", "sparse")


@functools.lru_cache(maxsize=None)
def float_grads(B, H, Wv, kind):
    """The pooled gradient G (B, 64, H / 2, 352) (1e30 in its pad columns), a random argmax (0 / 1 / 2 mixed in its pad columns)
    and the routed dz.  gauss: 1e-3 N(0, 1); heavy: 2^-k, k = 0..14; sparse: the Gaussian with seven planes of eight exactly 0."""
    g = np.random.default_rng(B * 10000 + H * 1000 + Wv + 31 + GRAD_KINDS.index(kind))
    Hp = H // 2
    Gv = heavy_tailed(g, (B, CO, Hp, Wv)) if kind == "heavy" else (g.standard_normal((B, CO, Hp, Wv)) * 1e-3).astype(f32)
    if kind == "sparse":
        Gv = Gv * (np.arange(B * CO).reshape(B, CO, 1, 1) % 8 == 3)
    amax = g.integers(0, 2, (B, CO, Hp, Wv)).astype(np.uint8)
    return _freeze(dict(G=planes(Gv.astype(f32), Wv), amax=poisoned_amax(g, amax, Wv), dz=route(Gv, amax)))


@functools.lru_cache(maxsize=None)
def float_fwd(B, H, Wv, Cin, T):
    """-> out, amax, z, zbound (Gate A per element of z), bound (Gate A of the pooled output), decided (where the argmax is
    held to the reference's)."""
    p = float_problem(B, H, Wv, Cin)
    W = p["W"].astype(f64)
    z = conv64(p["xhat"], W, T)
    pooled, amax = pool21(z)
    out = pooled + p["bias"].astype(f64)[None, :, None, None]
    zb = gamma(TAPS * Cin + 1) * conv64(np.abs(p["xhat"]), np.abs(W), T) + gamma(3) * conv64(p["xhat_mag"], np.abs(W), T)
    decided = np.abs(z[:, :, 1::2] - z[:, :, 0::2]) > BAND * np.abs(z).max()
    assert 1.0 - decided.mean() <= BAND_SHARE, (B, H, Wv, Cin, T, int((~decided).sum()))
    return _freeze(dict(out=out, amax=amax, z=z, zbound=zb, bound=np.maximum(zb[:, :, 0::2], zb[:, :, 1::2]) + U * np.abs(out),
                        decided=decided))


@functools.lru_cache(maxsize=None)
def float_dgrad(B, H, Wv, T, kind):
    W = float_problem(B, H, Wv, 64)["W"].astype(f64)
    dz = float_grads(B, H, Wv, kind)["dz"]
    return _freeze(dict(dx=conv64_dgrad(dz, W, T), bound=gamma(TAPS * CO + 1) * conv64_dgrad(np.abs(dz), np.abs(W), T)))


@functools.lru_cache(maxsize=None)
def float_wgrad(B, H, Wv, Cin, T, kind):
    p, dz = float_problem(B, H, Wv, Cin), float_grads(B, H, Wv, kind)["dz"]
    mag = conv64_wgrad(np.abs(dz), np.abs(p["xhat"]), T)
    return _freeze(dict(dW=conv64_wgrad(dz, p["xhat"], T),
                        bound=(gamma(B * H * Wv + 1) + 2 * U) * mag + gamma(3) * conv64_wgrad(np.abs(dz), p["xhat_mag"], T)))


def gate_b(kind, ref):
    """Gate B's bound: the same for every element."""
    return GATE_B[kind] * float(np.abs(ref).max())


# ---- statistics and plane sums ----------------------------------------------------------------------------------------------
EPS = float(np.float32(1e-5))                                                 # the kernel takes eps as a float


def stats_problem(B, C, H, Wv, with_slope):
    """Planes (B, C, H, 352) for mx_plane_stats / mx_plane_sum: Gaussian, but plane 0 exactly constant (negative: on the slope
    branch), plane 1 with mean / std = 1e3 and, where there is one, plane 2 with mean / std = -1e3."""
    g = np.random.default_rng(((B * 100 + C) * 100 + H) * 1000 + Wv + int(with_slope))
    x = (g.standard_normal((B * C, H, Wv)) * 0.7 + 0.1).astype(f32)
    x[0] = f32(-0.3)
    x[1] = (1.0e3 + g.standard_normal((H, Wv))).astype(f32)
    if B * C > 2:
        x[2] = (-1.0e3 + g.standard_normal((H, Wv))).astype(f32)
    slope = g.uniform(0.05, 0.45, C).astype(f32) if with_slope else None
    return planes(x.reshape(B, C, H, Wv), Wv), slope


def stats_ref(x, slope, Wv):
    """-> (stats (B, C, 2) fp64, bound (B, C, 2)) of mx_plane_stats.

    The kernel's arithmetic: t = fl32(slope x) on the slope branch (relative error <= 2^-24 =: v; identity otherwise); fp64 sums
    s, ss of the n = H Wv terms t, t^2 (w = 2^-53: gamma64(k) = k w / (1 - k w)); mean = s / n; var = max(ss / n - mean^2, 0);
    rstd = 1 / sqrt(var + eps); one rounding of each to fp32 (v).  With A = mean |t|, Q = mean t^2 of the reference's fp64 t:
    * the rounded terms t' = t + e, |e| <= v |t|, move the mean by at most v A and the variance by 2 cov(t, e) + var(e), at
      most 2 sqrt(var) v sqrt(Q) + v^2 Q (Cauchy-Schwarz; rms(e) <= v sqrt(Q));
    * the fp64 evaluation adds gamma64(n + 2) A to the mean and gamma64(n + 6) (Q + mean^2) to the variance (the sums, the
      squares, the two divisions, the subtraction -- every term is bounded by Q (1 + v)^2 or mean^2, which the + 6 absorbs); the
      clamp at 0 only moves the variance towards the true one, which is >= 0;
    * d(rstd) <= dvar / 2 (var + eps - dvar)^(3/2) (mean value theorem, the derivative taken at the worst point), the square
      root, the division and the sum with eps add 4 w rstd, the conversion v rstd.
    No slope: e = 0.  An exactly constant plane has var = 0 and dvar ~ 1e-12: rstd = 1 / sqrt(eps) to v."""
    xv = np.asarray(x, f64)[..., :Wv]
    t = xv if slope is None else prelu(xv, np.asarray(slope, f64)[None, :, None, None])
    ref = plane_stats(t, EPS)
    n = t.shape[2] * t.shape[3]
    v, w = (2.0 ** -24 if slope is not None else 0.0), 2.0 ** -53
    g64 = lambda k: k * w / (1.0 - k * w)
    A, Q = np.abs(t).mean((2, 3)), (t * t).mean((2, 3))
    mean, var = ref[..., 0], t.var((2, 3))
    dmean = v * A + g64(n + 2) * A + 2.0 ** -24 * np.abs(mean)
    dvar = 2 * np.sqrt(var) * v * np.sqrt(Q) + v * v * Q + g64(n + 6) * (Q + mean * mean)
    assert (dvar < 0.5 * (var + EPS)).all()
    drstd = 0.5 * dvar * (var + EPS - dvar) ** -1.5
    drstd = drstd + (2.0 ** -24 + 4 * w) * (ref[..., 1] + drstd)
    return ref, np.stack([dmean, drstd], -1)


def sum_ref(x, Wv):
    """-> (sums (planes,) fp64, bound) of mx_plane_sum: the fp64 sum of n terms (gamma64(n) of the sum of magnitudes) rounded
    once to fp32 (2^-24 of the sum)."""
    xv = np.asarray(x, f64)[..., :Wv]
    n = xv.shape[-2] * Wv
    s, mag = xv.sum((-2, -1)), np.abs(xv).sum((-2, -1))
    return s, 2.0 ** -24 * np.abs(s) + n * 2.0 ** -53 / (1 - n * 2.0 ** -53) * mag


# ---- an fp32 emulation of the three kernels' arithmetic ------------------------------------------------------------------------
def _tf32(a):
    """Round-toward-zero to a 10-bit mantissa."""
    return (np.ascontiguousarray(a, f32).view(np.uint32) & np.uint32(0xFFFFE000)).view(f32)


def _xhat32(p, defect):
    """The transformed input on all 352 columns, every operation rounded to fp32: PReLU product, - mean, * rstd."""
    x, stats = np.asarray(p["x"], f32), np.asarray(p["stats"], f32)
    if defect == "stats_of_clip_0":
        stats = np.broadcast_to(stats[:1], stats.shape)
    t = x
    if p.get("slope") is not None and defect != "prelu_skipped":
        t = np.where(x > 0, x, (np.asarray(p["slope"], f32)[None, :, None, None] * x).astype(f32))
    return ((t - stats[:, :, 0, None, None]).astype(f32) * stats[:, :, 1, None, None]).astype(f32)


def _dz32(p, defect):
    """The routed gradient on all 352 columns and 2 Hp rows."""
    G, amax = np.asarray(p["G"], f32), np.asarray(p["amax"])
    B, C, Hp, _ = G.shape
    dz = np.zeros((B, C, 2 * Hp, PITCH), f32)
    for r in range(2):
        dz[:, :, r::2] = G if defect == "route_ignores_amax" else np.where(amax == r, G, f32(0))
    return dz


def _window(plane, b, h, w, T, Wv, defect):
    """plane (B, C, H, 352) -> (n, C, 5, 13): plane[b][c][h + kh - 2][w + (kw - 6) T], zero outside the image and (but for
    pad_leaks) in the pad columns."""
    H = plane.shape[2]
    sh = lambda v: np.asarray(v)[:, None, None, None]
    c, kh, kw = np.arange(plane.shape[1])[None, :, None, None], np.arange(KH)[None, None, :, None], np.arange(KW)[None, None, None, :]
    rows = sh(h) + kh - 2
    dil = np.where(kw == KW - 1, T // 2, T) if defect == "last_tap_half_dilation" else T
    cols = sh(w) + (kw - 6) * dil
    lo_r, lo_c = (-1 if defect == "halo_row" else 0), (-1 if defect == "halo_col" else 0)
    ok = (rows >= lo_r) & (rows < H) & (cols >= lo_c) & (cols < (PITCH if defect == "pad_leaks" else Wv))
    return np.where(ok, plane[sh(b), c, np.clip(rows, 0, H - 1), np.clip(cols, 0, PITCH - 1)], f32(0))


def _fma_chain(a, b, order, defect):
    """(n, K) fp32 operands -> (n,) fp32: acc = fl32(acc + a_k b_k) (the product exact, as in a fused multiply-add), k ascending
    ("natural") or descending ("reversed")."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    if defect == "operands_truncated_to_tf32":
        a, b = _tf32(a), _tf32(b)
    keep = ((a != 0) & (b != 0)).any(0)                                       # adding an exact zero rounds nothing
    with np.errstate(over="ignore", invalid="ignore"):
        prod = a[:, keep].astype(f64) * b[:, keep].astype(f64)
        if order == "reversed":
            prod = prod[:, ::-1]
        else:
            assert order == "natural"
        acc = np.zeros(a.shape[0], f32)
        for k in range(prod.shape[1]):
            acc = (acc.astype(f64) + prod[:, k]).astype(f32)
    return acc


def emulate(kind, p, T, Wv, sel, order="natural", defect=None, rows_per_slab=3, grads=None):
    """One fp32 kernel on the tensors it is handed, for the outputs ``sel`` names; CPU only.
    kind "fwd":   p = x, stats, slope (None: first layer), W, bias;      sel (b, co, hp, w) -> (out fp32, amax uint8)
    kind "dgrad": grads = G, amax; p = W (64, 64, 5, 13);                sel (b, ci, h, w)  -> dxhat fp32
    kind "wgrad": grads = G, amax; p = x, stats, slope;                  sel (co, ci, kh, kw) -> dW fp32 (slab partials in
                  fp32, their sum in fp64, one conversion)
    ``defect``: one of DEFECTS (tests/test_f32block_refs64.py::test_defects_are_seen)."""
    assert defect is None or defect in DEFECTS
    sel = [np.asarray(s, np.int64) for s in sel]
    n = len(sel[0])
    W = np.asarray(p["W"], f32) if "W" in p else None
    if kind == "fwd":
        b, co, hp, w = sel
        xh = _xhat32(p, defect)
        rows = [_fma_chain(_window(xh, b, 2 * hp + r, w, T, Wv, defect).reshape(n, -1), W[co].reshape(n, -1), order, defect)
                for r in range(2)]
        take = rows[1] >= rows[0] if defect == "tie_takes_second" else rows[1] > rows[0]
        return (np.where(take, rows[1], rows[0]) + np.asarray(p["bias"], f32)[co]).astype(f32), take.astype(np.uint8)
    dz = _dz32(grads, defect)
    if kind == "dgrad":
        b, ci, h, w = sel
        Wk = W if defect == "taps_not_mirrored" else W[:, :, ::-1, ::-1]      # [co][ci][4 - kh][12 - kw]
        return _fma_chain(_window(dz, b, h, w, T, Wv, defect).reshape(n, -1), Wk[:, ci].transpose(1, 0, 2, 3).reshape(n, -1), order, defect)
    assert kind == "wgrad"
    co, ci, kh, kw = sel
    xh = _xhat32(p, defect)
    B, _, H, _ = xh.shape
    total = np.zeros(n)
    sh = lambda v: np.asarray(v)[:, None, None]
    for rid in slab_rows(B, H, rows_per_slab):
        if defect == "slab_last_row_dropped":
            rid = rid[:-1]
        if not len(rid):
            continue
        bb, hh, ww = (rid // H)[None, :, None], (rid % H)[None, :, None], np.arange(PITCH)[None, None, :]
        rows = hh + sh(kh) - 2 + 0 * ww
        dil = np.where(sh(kw) == KW - 1, T // 2, T) if defect == "last_tap_half_dilation" else T
        cols = ww + (sh(kw) - 6) * dil + 0 * hh
        lo_r, lo_c = (-1 if defect == "halo_row" else 0), (-1 if defect == "halo_col" else 0)
        lim = PITCH if defect == "pad_leaks" else Wv
        okx = (rows >= lo_r) & (rows < H) & (cols >= lo_c) & (cols < lim)
        xa = np.where(okx, xh[bb, sh(ci), np.clip(rows, 0, H - 1), np.clip(cols, 0, PITCH - 1)], f32(0))
        da = np.where(ww < lim, dz[bb, sh(co), hh, ww], f32(0))
        total += _fma_chain(da.reshape(n, -1), xa.reshape(n, -1), order, defect).astype(f64)
    with np.errstate(over="ignore"):
        return total.astype(f32)

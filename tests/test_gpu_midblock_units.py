"""GPU: the f16x3 kernels of the five 64 -> 64 channel blocks on their raw entry points, held to the independent fp64 references
of tests/helpers/midblock_refs64.py -- mx_conv_pack_weights_f16, mx_conv_pack_weights_sp_f16, mx_conv_prep_fwd_f16,
mx_conv_prep_dgrad_f16, mx_conv_prep_gpool_cl_f16, mx_conv_block_fwd_f16, mx_conv_block_dgrad_f16, mx_conv_block_dgrad_sp_f16,
mx_conv_block_wgrad_f16, mx_conv_block_wgrad_sp_f16, mx_ln_bwd_finish, mx_ln_prelu_bwd_gpool_f16 (conv_f16.hip,
dgrad_sp_f16.hip, wgrad_f16.hip, wgrad_sp_f16.hip).  tests/test_gpu_conv_units.py stays the chain test of the family.

Conventions of tests/test_gpu_block1_units.py: every output lives between two guard bands pre-filled with a NaN bit pattern
that must survive; the pad columns of every fp32 input hold 1e30 (the fp16 operand pairs keep +0 there: that is their
contract, asserted on what the preparation kernels write); every launch has valid arguments; every tolerance gate is
``worst ratio to its bound <= tol``.  u = 2^-23, gamma(n) = n u / (1 - n u).

* layouts: the packed weights and the index words equal the helpers' bit for bit;
* exact tests: hi operands are multiples of 8, lo operands small integers, so that every product and every partial sum is an
  integer below 2^24 (asserted from the fp64 sums of magnitudes where the references are formed): the fp32 accumulation of
  the matrix instructions, dense or sparse, is then exact in ANY order, and the result must equal the fp64 reference bit for
  bit -- one dropped split product, halo row, tap, slab or index bit shows (tests/test_midblock_refs64.py::test_defects_are_seen);
* rounding tests: the project's 1e-5 of the tensor's maximum, and per element (3 x 2^-22 + gamma(n + 2)) of the sum of the
  magnitudes of the n accumulated products plus what the absolute part 2^-25 of each pair contributes (midblock_refs64:
  float_fwd, float_dgrad, float_wgrad; tests/test_midblock_refs64.py holds the emulated arithmetic to the same bounds).
"""
import numpy as np
import pytest
import torch

from tests.helpers import block1_refs64 as R
from tests.helpers import midblock_refs64 as M
from tests.helpers.gpu_harness import (ARG, POISON, U, UNSUPPORTED, Out, bits, bits16, call, dv, f16, f32, f64, pair_ok, ratio,
                                       relmax, status)

pytestmark = pytest.mark.gpu
P = M.PITCH
gamma = M.gamma
N_PART = M.TAPS * 64 * 64                      # floats of one slab's partial result
OPN = 4 * P * 16                               # halfs of one row of a channels-last operand


def dv16(dev, a):
    """uint16 words to the device."""
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).to(dev)


def same_bits(got, want):
    """Number of fp32 elements whose bit patterns differ."""
    return int((bits(got) != bits(want)).sum())


def same_bits16(got, want):
    return int((bits16(got) != bits16(want)).sum())


# ==== layouts and operand preparation ========================================================================================
def test_pack_weights(dev):
    """W * 256 is exact in fp32, so hi = fp16(W * 256) and lo = fp16(W * 256 - hi) are determined bit for bit; the layouts
    are the header's (dense, flip 0 and 1; the sparse data gradient's fragment order with its structural zeros)."""
    g = np.random.default_rng(3)
    W = (g.standard_normal((64, 64, 5, 13)) / np.sqrt(4160)).astype(f32)
    W[0, 0, 0, 0], W[1, 1, 4, 12], W[63, 63, 2, 6] = 0.0, f32(2.0 ** -30), f32(-2.0 ** -30)  # a zero; W * 256 below the fp16 normal range
    Wd = dv(dev, W)
    for flip in (0, 1):
        hi_o, lo_o = Out(dev, M.W_ELEMS, f16), Out(dev, M.W_ELEMS, f16)
        call("mx_conv_pack_weights_f16", Wd, flip, hi_o, lo_o)
        hi, lo = M.split16(M.pack_weights(W, flip).astype(f32))
        assert hi_o.guards_intact() and lo_o.guards_intact()
        assert same_bits16(hi_o.read(), hi.ravel()) == 0 and same_bits16(lo_o.read(), lo.ravel()) == 0, flip
    hi_o, lo_o = Out(dev, M.W_SP_ELEMS, f16), Out(dev, M.W_SP_ELEMS, f16)
    call("mx_conv_pack_weights_sp_f16", Wd, hi_o, lo_o)
    hi, lo = M.split16(M.pack_weights_sp(W).astype(f32))
    assert hi_o.guards_intact() and lo_o.guards_intact()
    assert same_bits16(hi_o.read(), hi.ravel()) == 0 and same_bits16(lo_o.read(), lo.ravel()) == 0


@pytest.mark.parametrize("H", [2, 4, 6, 8])                                # H % 4 == 0: four rows per workgroup; else one
@pytest.mark.parametrize("Wv", [1, 17, 345, 351, 352])
def test_prep_fwd(dev, H, Wv):
    """The statistics are GIVEN (fp64 mean / rstd of PReLU(x) rounded to fp32): the kernel's arithmetic is the slope product,
    - mean, * rstd (3 fp32 operations) and the split."""
    g = np.random.default_rng(H * 1000 + Wv)
    B = 2
    x = np.full((B, 64, H, P), POISON, f32)
    x[..., :Wv] = (g.standard_normal((B, 64, H, Wv)) * 0.7 + 0.1).astype(f32)
    slope = g.uniform(0.05, 0.45, 64).astype(f32)
    y = M.prelu(x[..., :Wv].astype(f64), slope.astype(f64)[None, :, None, None])
    stats = M.plane_stats(y).astype(f32)
    hi_o, lo_o = Out(dev, B * H * OPN, f16), Out(dev, B * H * OPN, f16)
    call("mx_conv_prep_fwd_f16", dv(dev, x), dv(dev, stats), dv(dev, slope), B, H, Wv, hi_o, lo_o)
    hi, lo = hi_o.read().reshape(B, H, 4, P, 16), lo_o.read().reshape(B, H, 4, P, 16)
    assert hi_o.guards_intact() and lo_o.guards_intact()
    assert not bits16(hi[:, :, :, Wv:]).any() and not bits16(lo[:, :, :, Wv:]).any()           # pad columns: exactly +0
    m, r = stats.astype(f64)[:, :, 0, None, None], stats.astype(f64)[:, :, 1, None, None]
    v64, mag = M.cl_layout(M.normalise(y, stats), Wv), M.cl_layout((np.abs(y) + np.abs(m)) * r, Wv)
    tol = 1.0
    assert pair_ok(hi, lo, v64, 3 * U * mag) <= tol


_PREP_SHAPES = [(1, 2, 17), (2, 8, 345), (3, 6, 352), (2, 4, 1)]


def _grad_input(B, H, Wv, kind, seed):
    g = np.random.default_rng(seed)
    Hp = H // 2
    G = np.full((B, 64, Hp, P), POISON, f32)
    G[..., :Wv] = M.heavy_tailed(g, (B, 64, Hp, Wv)) if kind == "heavy" else (g.standard_normal((B, 64, Hp, Wv)) * 1e-3).astype(f32)
    return G, g.integers(0, 2, (B, 64, Hp, P)).astype(np.uint8)


@pytest.mark.parametrize("kind", ["gauss", "heavy"])
@pytest.mark.parametrize("B,H,Wv", _PREP_SHAPES)
def test_prep_dgrad(dev, B, H, Wv, kind):
    """S is the power of two that puts max |G| S into [512, 1024) -- over the valid columns: the pads hold 1e30; G * S is exact,
    so the routed pair is determined bit for bit; pad columns exactly +0; amax_ready = 1 (the bits of max |G| handed in)
    agrees with the sweep; dz_hi = dz_lo = NULL leaves the scale alone."""
    G, amax = _grad_input(B, H, Wv, kind, B * 100 + H + Wv)
    gmax = np.abs(G[..., :Wv]).max()
    S = M.pow2_scale(gmax)
    assert 512.0 <= float(gmax) * S < 1024.0
    hi, lo = (M.cl_layout(h, Wv) for h in M.split16((M.route(G[..., :Wv], amax[..., :Wv]) * S).astype(f32)))
    Gd, ad = dv(dev, G), dv(dev, amax, np.uint8)
    for ready in (0, 1):
        ws = Out(dev, 1, np.uint32, init=bits(np.array([gmax], f32)) if ready else None)
        scale, hi_o, lo_o = Out(dev, 2), Out(dev, B * H * OPN, f16), Out(dev, B * H * OPN, f16)
        call("mx_conv_prep_dgrad_f16", Gd, ad, B, H, Wv, ws, ready, scale, hi_o, lo_o)
        for o in (ws, scale, hi_o, lo_o):
            assert o.guards_intact()
        assert scale.read().tolist() == [S, 1.0 / S], ready
        assert int(ws.read()[0]) == int(bits(np.array([gmax], f32))[0])
        assert same_bits16(hi_o.read(), hi.ravel()) == 0 and same_bits16(lo_o.read(), lo.ravel()) == 0, ready
    ws, scale = Out(dev, 1, np.uint32), Out(dev, 2)
    call("mx_conv_prep_dgrad_f16", Gd, ad, B, H, Wv, ws, 0, scale, None, None)
    assert scale.read().tolist() == [S, 1.0 / S] and scale.guards_intact() and ws.guards_intact()


def _gpool(dev, Gd, ad, scale_d, B, H, Wv, with_gidx=True):
    Hp = H // 2
    o = dict(g_hi=Out(dev, B * Hp * OPN, f16), g_lo=Out(dev, B * Hp * OPN, f16), g_idx=Out(dev, B * Hp * 4 * P, np.uint32))
    if with_gidx:
        o["gidx"] = Out(dev, B * 64 * Hp * 22 * 2, np.uint16)
    call("mx_conv_prep_gpool_cl_f16", Gd, ad, scale_d, B, H, Wv, o["g_hi"], o["g_lo"], o["g_idx"], o.get("gidx"))
    for v in o.values():
        assert v.guards_intact()
    return o


@pytest.mark.parametrize("shift", [0, 6])
@pytest.mark.parametrize("kind", ["gauss", "heavy"])
@pytest.mark.parametrize("B,H,Wv", _PREP_SHAPES)
def test_prep_gpool(dev, B, H, Wv, kind, shift):
    """The pooled pair is the split of G * S bit for bit (S handed in: the scale of the sweep, or 2^6 smaller as
    mx_ln_bwd_finish's bound may give), +0 in the pad columns; both kinds of index words equal the header's layouts on all 352
    positions; without gidx the rest is unchanged."""
    G, amax = _grad_input(B, H, Wv, kind, B * 100 + H + Wv + 1)
    S = M.pow2_scale(np.abs(G[..., :Wv]).max()) / 2.0 ** shift
    Gd, ad, sd = dv(dev, G), dv(dev, amax, np.uint8), dv(dev, np.array([S, 1.0 / S], f32))
    o = _gpool(dev, Gd, ad, sd, B, H, Wv)
    hi, lo = (M.cl_layout(h, Wv) for h in M.split16((G[..., :Wv].astype(f64) * S).astype(f32)))
    assert same_bits16(o["g_hi"].read(), hi.ravel()) == 0 and same_bits16(o["g_lo"].read(), lo.ravel()) == 0
    assert (lo != 0).any() or kind == "heavy"                                 # (powers of two have no lo half)
    assert np.array_equal(o["g_idx"].read(), M.g_idx_words(amax).ravel())
    assert np.array_equal(o["gidx"].read(), M.gidx_words(amax).ravel())
    o2 = _gpool(dev, Gd, ad, sd, B, H, Wv, with_gidx=False)
    for k in ("g_hi", "g_lo", "g_idx"):
        assert torch.equal(o[k].body_words(), o2[k].body_words())


# ==== exact on integers =========================================================================================================
_CASES = [(s, T) for s in M.EXACT_SHAPES_DENSE for T in M.DILATIONS]
_ids = lambda c: f"{c[0][0]}x{c[0][1]}x{c[0][2]}-T{c[1]}"
# what the shapes are chosen for (midblock_refs64.EXACT_SHAPES)
assert {B * (H // 2) % 8 == 0 for B, H, _ in M.EXACT_SHAPES} == {True, False} and any(H == 2 for _, H, _ in M.EXACT_SHAPES)
assert any(B == 1 for B, _, _ in M.EXACT_SHAPES) and any(Wv < 6 for _, _, Wv in M.EXACT_SHAPES)


@pytest.mark.parametrize("case", _CASES, ids=_ids)
def test_fwd_exact_on_integers(dev, case):
    """x_hi = 8 a, x_lo = b, w_hi = 8 c, w_lo = d (|a|, |b|, |c|, |d| <= 3), bias a multiple of 1 / 256: out must equal
    (sum hi hi + hi lo + lo hi) / 256 + bias bit for bit and the argmax plane exactly (ties: the even row; the last clip has all
    rows alike), pad columns +0, with and without the optional statistics.  Dilations 1, 2, 4 run the LDS-DMA kernel, 8 and 16
    the register-staged one; B * H / 2 a multiple of 8 takes the workgroup renumbering."""
    (B, H, Wv), T = case
    i, w, ref = M.exact_inputs(B, H, Wv), M.exact_weights(), M.exact_fwd(B, H, Wv, T)
    assert ref["ties"] > 0 or H < 6 or B == 1
    Hp = H // 2
    n = B * 64 * Hp * P
    ops = [dv(dev, a, f16) for a in (i["x_hi"], i["x_lo"], w["fwd_hi"], w["fwd_lo"])] + [dv(dev, i["bias"])]
    slope = np.random.default_rng(1).uniform(0.05, 0.5, 64).astype(f32)
    out_s, am_s, sp = Out(dev, n), Out(dev, n, np.uint8), Out(dev, B * Hp * 64 * 2)
    call("mx_conv_block_fwd_f16", *ops, B, H, Wv, T, out_s, am_s, dv(dev, slope), sp)
    out_n, am_n = Out(dev, n), Out(dev, n, np.uint8)
    call("mx_conv_block_fwd_f16", *ops, B, H, Wv, T, out_n, am_n, None, None)
    for o in (out_s, am_s, sp, out_n, am_n):
        assert o.guards_intact()
    assert torch.equal(out_s.body_words(), out_n.body_words()) and torch.equal(am_s.body_words(), am_n.body_words())
    got = out_s.read().reshape(B, 64, Hp, P)
    assert not bits(got[..., Wv:]).any()                                      # pad columns: written as +0
    bad = np.argwhere(bits(got[..., :Wv]) != bits(ref["out"]))
    assert bad.shape[0] == 0, (bad.shape[0], bad[:4].tolist(), [float(got[tuple(k)]) for k in bad[:4]], [float(ref["out"][tuple(k)]) for k in bad[:4]])
    gam = am_s.read().reshape(B, 64, Hp, P)[..., :Wv]
    assert np.array_equal(gam, ref["amax"]), np.argwhere(gam != ref["amax"])[:4].tolist()
    # the optional by-product: row sums of PReLU(out) - PReLU(bias) and of its square over w < Wv
    want, mag = R.stats_rows(ref["out"], i["bias"], slope)
    gsp = sp.read().reshape(B, Hp, 64, 2)
    tol = 1.0
    # Wv terms + 1, and per term the slope product, the shift's own product and the subtraction: gamma(Wv + 4);
    # squares: the error of d enters twice (2 x 3), the square rounds once: gamma(Wv + 8) of sum (|PReLU(out)| + |PReLU(bias)|)^2
    assert ratio(gsp[..., 0], want[..., 0], gamma(Wv + 4) * mag[..., 0]) <= tol
    assert ratio(gsp[..., 1], want[..., 1], gamma(Wv + 8) * mag[..., 1]) <= tol


@pytest.mark.parametrize("case", _CASES, ids=_ids)
def test_dgrad_exact_on_integers(dev, case):
    """g_hi = 8 a, g_lo = b routed by a random argmax, S = 4: dxhat of the dense kernel (routed pair, flipped weights) and of
    the sparse kernel (pooled pair, index words, fragment-ordered weights; Wv <= 351) must equal the fp64 reference bit for
    bit -- hence each other -- with +0 pad columns; the sparse kernel's LayerNorm partial sums and maxima leave dxhat as it is."""
    (B, H, Wv), T = case
    i, w, o, ref = M.exact_inputs(B, H, Wv), M.exact_weights(), M.exact_grad_operands(B, H, Wv), M.exact_dgrad(B, H, Wv, T)
    n = B * 64 * H * P
    scale = dv(dev, i["scale"])

    def check(out, what):
        assert out.guards_intact()
        got = out.read().reshape(B, 64, H, P)
        assert not bits(got[..., Wv:]).any(), what
        bad = np.argwhere(bits(got[..., :Wv]) != bits(ref["dx"]))
        assert bad.shape[0] == 0, (what, bad.shape[0], bad[:4].tolist(), [float(got[tuple(k)]) for k in bad[:4]],
                                   [float(ref["dx"][tuple(k)]) for k in bad[:4]])

    dense = Out(dev, n)
    call("mx_conv_block_dgrad_f16", dv(dev, o["dz_hi"], f16), dv(dev, o["dz_lo"], f16), dv(dev, w["flip_hi"], f16), dv(dev, w["flip_lo"], f16),
         scale, B, H, Wv, T, dense)
    check(dense, "dense")
    if Wv > P - 1:
        return
    sp_ops = [dv(dev, o["g_hi"], f16), dv(dev, o["g_lo"], f16), dv(dev, o["g_idx"], np.uint32), dv(dev, w["sp_hi"], f16), dv(dev, w["sp_lo"], f16),
              scale, B, H, Wv, T]
    plain = Out(dev, n)
    call("mx_conv_block_dgrad_sp_f16", *sp_ops, plain, None, None, None, None)
    check(plain, "sparse")
    assert torch.equal(plain.body_words(), dense.body_words())
    x_hi, x_lo = dv(dev, i["x_hi"], f16), dv(dev, i["x_lo"], f16)
    with_ln, ln_part = Out(dev, n), Out(dev, B * 64 * H * 2 * 2)
    call("mx_conv_block_dgrad_sp_f16", *sp_ops, with_ln, x_hi, x_lo, ln_part, None)
    with_gx, ln_part2, gx = Out(dev, n), Out(dev, B * 64 * H * 2 * 2), Out(dev, 2, np.uint32, init=np.zeros(2, np.uint32))
    call("mx_conv_block_dgrad_sp_f16", *sp_ops, with_gx, x_hi, x_lo, ln_part2, gx)
    for out in (with_ln, ln_part, with_gx, ln_part2, gx):
        assert out.guards_intact()
    assert torch.equal(with_ln.body_words(), plain.body_words()) and torch.equal(with_gx.body_words(), plain.body_words())
    assert torch.equal(ln_part.body_words(), ln_part2.body_words())
    # {sum dxhat, sum dxhat xhat} per (plane, row, position half): which half takes the middle tile depends on the wave, so
    # the sum over both halves is pinned.  Wv additions (+ 1 joining the halves), and per term the product: gamma(Wv + 4)
    d, xv = ref["dx"].astype(f64), i["xh"] + i["xl"]
    want = np.stack([d.sum(-1), (d * xv).sum(-1)], -1)
    mag = np.stack([np.abs(d).sum(-1), (np.abs(d) * np.abs(xv)).sum(-1)], -1)
    got = ln_part.read().reshape(B, 64, H, 2, 2).astype(f64).sum(3)
    tol = 1.0
    assert ratio(got, want, gamma(Wv + 4) * mag) <= tol
    assert gx.read().tolist() == bits(np.array([np.abs(ref["dx"]).max(), np.abs(xv).max()], f32)).tolist()


def _slab_choices(rows):
    """rows_per_slab values: one slab for everything (larger than all rows), three slabs, and 2 and 1 rows per slab."""
    return sorted({rows + 3, -(-rows // 3), 2, 1})


# what the shapes and _slab_choices give: n_slabs of 1, 3 (fewer than the reduce kernel's four quarters), 8 and 9 (one workgroup
# of the second group of eight; the rest idle), more than 8 and no multiple of 8, a short last slab, slabs that span two clips
_DENSE_SLABS = {-(-(B * H) // r) for B, H, _ in M.EXACT_SHAPES_DENSE for r in _slab_choices(B * H)}
_SPARSE_SLABS = {-(-(B * (H // 2)) // r) for B, H, _ in M.EXACT_SHAPES for r in _slab_choices(B * (H // 2))}
assert {1, 3, 8, 9, 18} <= _DENSE_SLABS and {1, 3, 8, 9} <= _SPARSE_SLABS
assert (3, 6, 40) in M.EXACT_SHAPES and 9 % 2 == 1 and 9 % 4 == 1             # H / 2 = 3: 2-row slabs span clips, the last is short


def _wgrad_run(dev, entry, args, rows, rps):
    n_slabs = -(-rows // rps)
    part, dW = Out(dev, n_slabs * N_PART), Out(dev, 64 * 64 * M.TAPS)
    call(entry, *args, rps, part, dW)
    assert part.guards_intact() and dW.guards_intact()
    assert part.untouched() == 0 and dW.untouched() == 0, (entry, rps)
    return dW.read().reshape(64, 64, 5, 13)


@pytest.mark.parametrize("case", _CASES, ids=_ids)
def test_wgrad_exact_on_integers(dev, case):
    """Integer operands, S = 4, every slab sum exact: dW of the dense kernel (routed pair) and of the sparse kernel (pooled
    pair + planar index words; Wv <= 351) must equal the fp64 reference rounded once to fp32 bit for bit, for every
    rows_per_slab of _slab_choices."""
    (B, H, Wv), T = case
    i, o, ref = M.exact_inputs(B, H, Wv), M.exact_grad_operands(B, H, Wv), M.exact_wgrad(B, H, Wv, T)
    x_hi, x_lo, scale = dv(dev, i["x_hi"], f16), dv(dev, i["x_lo"], f16), dv(dev, i["scale"])
    dense = [dv(dev, o["dz_hi"], f16), dv(dev, o["dz_lo"], f16), x_hi, x_lo, scale, B, H, T]
    for rps in _slab_choices(B * H):
        got = _wgrad_run(dev, "mx_conv_block_wgrad_f16", dense, B * H, rps)
        bad = np.argwhere(bits(got) != bits(ref["dW"]))
        assert bad.shape[0] == 0, ("dense", rps, bad.shape[0], bad[:4].tolist(), [float(got[tuple(k)]) for k in bad[:4]],
                                   [float(ref["dW"][tuple(k)]) for k in bad[:4]])
    if Wv > P - 1:
        return
    sparse = [dv(dev, o["g_hi"], f16), dv(dev, o["g_lo"], f16), dv16(dev, o["gidx"]), x_hi, x_lo, scale, B, H, Wv, T]
    for rps in _slab_choices(B * (H // 2)):
        got = _wgrad_run(dev, "mx_conv_block_wgrad_sp_f16", sparse, B * (H // 2), rps)
        bad = np.argwhere(bits(got) != bits(ref["dW"]))
        assert bad.shape[0] == 0, ("sparse", rps, bad.shape[0], bad[:4].tolist(), [float(got[tuple(k)]) for k in bad[:4]],
                                   [float(ref["dW"][tuple(k)]) for k in bad[:4]])


# ==== rounding on floats ==========================================================================================================
def _device_weights(dev, W):
    Wd = dv(dev, W)
    o = {}
    for name, n, entry, args in (("wf", M.W_ELEMS, "mx_conv_pack_weights_f16", (0,)), ("wflip", M.W_ELEMS, "mx_conv_pack_weights_f16", (1,)),
                                 ("wsp", M.W_SP_ELEMS, "mx_conv_pack_weights_sp_f16", ())):
        o[name] = (Out(dev, n, f16), Out(dev, n, f16))
        call(entry, Wd, *args, *o[name])
    return o


@pytest.mark.parametrize("T", M.DILATIONS)
@pytest.mark.parametrize("B,H,Wv", M.ROUNDING_SHAPES)
def test_rounding_on_random_floats(dev, B, H, Wv, T):
    """Every operand is prepared by the device kernels from random fp32 inputs (1e30 in their pad columns); the five conv
    entry points against the fp64 references on the same fp32 inputs.  Bounds: midblock_refs64.float_fwd / float_dgrad /
    float_wgrad -- n = 3 x 4160 products per output of the convolutions, 3 x (rows of a slab) x Wv per slab of the weight
    gradients.  Gradients: Gaussian and heavy-tailed (2^-k, k = 0..14), each on the scale mx_conv_prep_dgrad_f16 picks and, for
    the pooled operand of the sparse kernels, on one 2^6 smaller."""
    i = M.float_inputs(B, H, Wv)
    Hp = H // 2
    wk = _device_weights(dev, i["W"])
    x_hi, x_lo = Out(dev, B * H * OPN, f16), Out(dev, B * H * OPN, f16)
    call("mx_conv_prep_fwd_f16", dv(dev, i["x"]), dv(dev, i["stats"]), dv(dev, i["slope"]), B, H, Wv, x_hi, x_lo)
    tol = 1.0
    # ---- forward
    ref = M.float_fwd(B, H, Wv, T)
    n = B * 64 * Hp * P
    out, am = Out(dev, n), Out(dev, n, np.uint8)
    call("mx_conv_block_fwd_f16", x_hi, x_lo, *wk["wf"], dv(dev, i["bias"]), B, H, Wv, T, out, am, None, None)
    got = out.read().reshape(B, 64, Hp, P)
    assert out.guards_intact() and am.guards_intact() and x_hi.guards_intact() and x_lo.guards_intact()
    assert not bits(got[..., Wv:]).any()
    zb = ref["zbound"]
    bound = np.maximum(zb[:, :, 0::2], zb[:, :, 1::2]) + U * np.abs(i["bias"].astype(f64))[None, :, None, None]
    assert relmax(got[..., :Wv], ref["out"]) < 1e-5
    assert ratio(got[..., :Wv], ref["out"], bound) <= tol
    # the argmax may differ from the reference's only where the two rows are closer than their bounds together
    z = ref["z"]
    diff = am.read().reshape(B, 64, Hp, P)[..., :Wv] != ref["amax"]
    assert (np.abs(z[:, :, 1::2] - z[:, :, 0::2])[diff] <= (zb[:, :, 0::2] + zb[:, :, 1::2])[diff]).all(), int(diff.sum())
    # ---- gradients
    for kind in ("gauss", "heavy"):
        gi = M.float_inputs(B, H, Wv, kind)
        Gd, ad = dv(dev, gi["G"]), dv(dev, gi["amax"], np.uint8)
        ws, scale, dz_hi, dz_lo = Out(dev, 1, np.uint32), Out(dev, 2), Out(dev, B * H * OPN, f16), Out(dev, B * H * OPN, f16)
        call("mx_conv_prep_dgrad_f16", Gd, ad, B, H, Wv, ws, 0, scale, dz_hi, dz_lo)
        S = float(scale.read()[0])
        assert S == M.float_dgrad(B, H, Wv, T, kind, 0)["S"]
        dref, wref = M.float_dgrad(B, H, Wv, T, kind, 0), M.float_wgrad(B, H, Wv, T, kind, 0)
        dx = Out(dev, B * 64 * H * P)
        call("mx_conv_block_dgrad_f16", dz_hi, dz_lo, *wk["wflip"], scale, B, H, Wv, T, dx)
        got = dx.read().reshape(B, 64, H, P)
        assert dx.guards_intact() and not bits(got[..., Wv:]).any()
        assert relmax(got[..., :Wv], dref["dx"]) < 1e-5
        assert ratio(got[..., :Wv], dref["dx"], dref["bound"]) <= tol
        rps = 3
        got = _wgrad_run(dev, "mx_conv_block_wgrad_f16", [dz_hi, dz_lo, x_hi, x_lo, scale, B, H, T], B * H, rps)
        assert relmax(got, wref["dW"]) < 1e-5
        assert ratio(got, wref["dW"], M.wgrad_bound(wref, 3 * rps * Wv)) <= tol
        for shift in (0, 6):
            dref, wref = M.float_dgrad(B, H, Wv, T, kind, shift), M.float_wgrad(B, H, Wv, T, kind, shift)
            sc = dv(dev, np.array([dref["S"], 1.0 / dref["S"]], f32))
            o = _gpool(dev, Gd, ad, sc, B, H, Wv)
            dx = Out(dev, B * 64 * H * P)
            call("mx_conv_block_dgrad_sp_f16", o["g_hi"], o["g_lo"], o["g_idx"], *wk["wsp"], sc, B, H, Wv, T, dx, None, None, None, None)
            got = dx.read().reshape(B, 64, H, P)
            assert dx.guards_intact() and not bits(got[..., Wv:]).any()
            assert relmax(got[..., :Wv], dref["dx"]) < 1e-5
            assert ratio(got[..., :Wv], dref["dx"], dref["bound"]) <= tol
            rps = 2                                                            # pooled rows: 4 image rows of Wv positions per slab
            got = _wgrad_run(dev, "mx_conv_block_wgrad_sp_f16", [o["g_hi"], o["g_lo"], o["gidx"], x_hi, x_lo, sc, B, H, Wv, T], B * Hp, rps)
            assert relmax(got, wref["dW"]) < 1e-5
            assert ratio(got, wref["dW"], M.wgrad_bound(wref, 3 * 2 * rps * Wv)) <= tol


# ==== the fused LayerNorm / PReLU backward into the pooled operand ==================================================================
@pytest.mark.parametrize("B,Hp,Wv", [(2, 4, 345), (1, 1, 17)])
def test_ln_bwd_finish_and_gpool(dev, B, Hp, Wv):
    """mx_ln_bwd_finish: m12 = the plane means from ln_part's fp32 partial sums (fp64 sums rounded once), S a power of two from a
    true bound on max |G| within 2^6 of it.  mx_ln_prelu_bwd_gpool_f16 on that scale against R.ln_prelu_bwd in fp64: the pair
    within the pair bound of G S plus the backward's own rounding (10 fp32 operations, as tests/test_gpu_block1_units.py counts
    them for mx_ln_prelu_bwd_pair); index words as the helpers'; the per-plane sums within gamma(Hp Wv + 14) of their magnitudes."""
    g = np.random.default_rng(31 * B + Hp + Wv)
    C = 64
    p, d = np.full((B, C, Hp, P), POISON, f32), np.full((B, C, Hp, P), POISON, f32)
    p[..., :Wv] = g.standard_normal((B, C, Hp, Wv)).astype(f32)
    p[:, :, 0, 0], p[:, 1::2, Hp - 1, Wv - 1] = 0.0, -0.0                      # the kink: the slope branch
    d[..., :Wv] = (g.standard_normal((B, C, Hp, Wv)) * 1e-2).astype(f32)
    slope = g.uniform(0.05, 0.5, C).astype(f32)
    amax = g.integers(0, 2, (B, C, Hp, P)).astype(np.uint8)
    pv, dvv = p[..., :Wv], d[..., :Wv]
    stats = R.plane_stats(R.prelu(pv.astype(f64), slope.astype(f64)[None, :, None, None])).astype(f32)
    xh = R.ln_prelu_bwd(pv, dvv, stats, slope)["xhat"]
    halves = [slice(0, min(192, Wv)), slice(min(192, Wv), Wv)]
    ln_part = np.stack([np.stack([dvv[..., s].astype(f64).sum(-1), (dvv[..., s] * xh[..., s]).sum(-1)], -1) for s in halves], -2).astype(f32)
    n = Hp * Wv
    m12_64 = np.stack([ln_part.astype(f64)[..., 0].sum((2, 3)) / n, ln_part.astype(f64)[..., 1].sum((2, 3)) / n], -1)
    gx = bits(np.array([np.abs(dvv).max(), np.abs(xh).max()], f32)).view(np.uint32)
    pd, dd, sd, sld = dv(dev, p), dv(dev, d), dv(dev, stats), dv(dev, slope)
    m12, bound_ws, scale = Out(dev, B * C * 2), Out(dev, 1, np.uint32), Out(dev, 2)
    call("mx_ln_bwd_finish", dv(dev, ln_part), sd, sld, dv(dev, gx, np.uint32), B, C, Hp, Wv, m12, bound_ws, scale)
    for o in (m12, bound_ws, scale):
        assert o.guards_intact()
    gm12 = m12.read().reshape(B, C, 2)
    tol = 1.0
    # fp64 sums of the 2 Hp partials and one division, rounded once to fp32 (u / 2 of the mean; the fp64 sum's own order: 2^-50)
    part_mag = np.stack([np.abs(ln_part.astype(f64))[..., 0].sum((2, 3)) / n, np.abs(ln_part.astype(f64))[..., 1].sum((2, 3)) / n], -1)
    assert ratio(gm12, m12_64, U / 2 * np.abs(m12_64) + 2.0 ** -50 * part_mag) <= tol
    ref = R.ln_prelu_bwd(pv, dvv, stats, slope, m12=(gm12[..., 0], gm12[..., 1]))
    S, inv = scale.read().tolist()
    gmax = float(np.abs(ref["G"]).max())
    assert S == 2.0 ** round(np.log2(S)) and inv == 1.0 / S and 16.0 <= gmax * S < 1024.0
    o = dict(g_hi=Out(dev, B * Hp * OPN, f16), g_lo=Out(dev, B * Hp * OPN, f16), g_idx=Out(dev, B * Hp * 4 * P, np.uint32),
             gidx=Out(dev, B * C * Hp * 22 * 2, np.uint16), part=Out(dev, B * C * Hp * 6 * 2), ds=Out(dev, B * C), gs=Out(dev, B * C))
    call("mx_ln_prelu_bwd_gpool_f16", pd, dd, dv(dev, amax, np.uint8), sd, sld, m12, scale, B, Hp, Wv, o["g_hi"], o["g_lo"], o["g_idx"],
         o["gidx"], o["part"], o["ds"], o["gs"])
    for v in o.values():
        assert v.guards_intact()
    hi, lo = o["g_hi"].read().reshape(B, Hp, 4, P, 16), o["g_lo"].read().reshape(B, Hp, 4, P, 16)
    assert not bits16(hi[:, :, :, Wv:]).any() and not bits16(lo[:, :, :, Wv:]).any()
    assert np.array_equal(o["g_idx"].read(), M.g_idx_words(amax).ravel()) and np.array_equal(o["gidx"].read(), M.gidx_words(amax).ravel())
    # fp32 operations of the formula: 10 (slope p, - mean, rstd; xhat m2, - m1, - , rstd, slope; the roundings of m1 and m2);
    # G S is exact; the pair adds 2^-22 |G S| + 2^-25 of the value the kernel computed (hence the 1 + 2^-22)
    want, mag = M.cl_layout(ref["G"] * S, Wv), M.cl_layout(ref["G_mag"] * S, Wv)
    assert pair_ok(hi, lo, want, 10 * U * mag * (1 + 2.0 ** -22)) <= tol
    # per-plane sums: fp32 over the 16 lanes of a channel and tile, fp64 over the tiles; their terms carry the elementwise
    # error (10), one more product and the additions of a tile: gamma(Hp Wv + 14) of the magnitudes is generous and safe
    assert ratio(o["ds"].read().reshape(B, C), ref["dslope"], gamma(Hp * Wv + 14) * ref["dslope_mag"]) <= tol
    assert ratio(o["gs"].read().reshape(B, C), ref["gsum"], gamma(Hp * Wv + 14) * ref["gsum_mag"]) <= tol


# ==== documented statuses ===========================================================================================================
def test_documented_statuses_without_a_launch(dev):
    """Every refusal happens before a launch: the outputs keep their sentinel words."""
    z = torch.zeros(1 << 16, device=dev)
    outs = []

    def out():
        outs.append(Out(dev, 1 << 12))
        return outs[-1]

    base = dict(B=1, H=2, Wv=8, T=1)

    def fwd(**k):
        a = dict(dict(base, x_hi=z, x_lo=z, w_hi=z, w_lo=z, bias=z, out=out(), amax=out(), slope=None, stats=None), **k)
        return status("mx_conv_block_fwd_f16", a["x_hi"], a["x_lo"], a["w_hi"], a["w_lo"], a["bias"], a["B"], a["H"], a["Wv"], a["T"],
                      a["out"], a["amax"], a["slope"], a["stats"])

    def dgrad(**k):
        a = dict(dict(base, dz_hi=z, dz_lo=z, w_hi=z, w_lo=z, scale=z, out=out()), **k)
        return status("mx_conv_block_dgrad_f16", a["dz_hi"], a["dz_lo"], a["w_hi"], a["w_lo"], a["scale"], a["B"], a["H"], a["Wv"], a["T"], a["out"])

    def dgrad_sp(**k):
        a = dict(dict(base, g_hi=z, g_lo=z, g_idx=z, w_hi=z, w_lo=z, scale=z, out=out(), x_hi=None, x_lo=None, ln_part=None, gx=None), **k)
        return status("mx_conv_block_dgrad_sp_f16", a["g_hi"], a["g_lo"], a["g_idx"], a["w_hi"], a["w_lo"], a["scale"], a["B"], a["H"], a["Wv"],
                      a["T"], a["out"], a["x_hi"], a["x_lo"], a["ln_part"], a["gx"])

    def wgrad(**k):
        a = dict(dict(base, dz_hi=z, dz_lo=z, x_hi=z, x_lo=z, scale=z, rps=1, part=out(), dW=out()), **k)
        return status("mx_conv_block_wgrad_f16", a["dz_hi"], a["dz_lo"], a["x_hi"], a["x_lo"], a["scale"], a["B"], a["H"], a["T"], a["rps"],
                      a["part"], a["dW"])

    def wgrad_sp(**k):
        a = dict(dict(base, g_hi=z, g_lo=z, gidx=z, x_hi=z, x_lo=z, scale=z, rps=1, part=out(), dW=out()), **k)
        return status("mx_conv_block_wgrad_sp_f16", a["g_hi"], a["g_lo"], a["gidx"], a["x_hi"], a["x_lo"], a["scale"], a["B"], a["H"], a["Wv"],
                      a["T"], a["rps"], a["part"], a["dW"])

    # sizes: Wv = 352 on both sparse kernels; odd H, H < 2; a dilation of 3
    assert dgrad_sp(Wv=352) == UNSUPPORTED and wgrad_sp(Wv=352) == UNSUPPORTED
    for entry in (fwd, dgrad, dgrad_sp, wgrad_sp):
        assert entry(H=3) == UNSUPPORTED and entry(H=0) == UNSUPPORTED and entry(T=3) == UNSUPPORTED, entry.__name__
    assert wgrad(T=3) == UNSUPPORTED and fwd(Wv=353) == UNSUPPORTED and dgrad(Wv=353) == UNSUPPORTED
    # arguments that need each other
    assert fwd(stats=z) == ARG                                                   # stats_part without slope_out
    assert dgrad_sp(gx=z) == ARG and dgrad_sp(x_hi=z, x_lo=z, gx=z) == ARG        # gx_bits without ln_part
    assert dgrad_sp(x_hi=z) == ARG and dgrad_sp(x_hi=z, x_lo=z) == ARG and dgrad_sp(ln_part=z) == ARG     # x_hi / x_lo / ln_part: all or none
    assert status("mx_conv_prep_dgrad_f16", z, z, 1, 2, 8, z, 0, out(), z, None) == ARG                   # dz_hi without dz_lo
    assert status("mx_conv_prep_dgrad_f16", z, z, 1, 2, 8, z, 0, out(), None, z) == ARG
    # every required pointer
    for entry, names in ((fwd, ("x_hi", "x_lo", "w_hi", "w_lo", "bias", "out", "amax")), (dgrad, ("dz_hi", "dz_lo", "w_hi", "w_lo", "scale", "out")),
                         (dgrad_sp, ("g_hi", "g_lo", "g_idx", "w_hi", "w_lo", "scale", "out")),
                         (wgrad, ("dz_hi", "dz_lo", "x_hi", "x_lo", "scale", "part", "dW")),
                         (wgrad_sp, ("g_hi", "g_lo", "gidx", "x_hi", "x_lo", "scale", "part", "dW"))):
        for name in names:
            assert entry(**{name: None}) == ARG, (entry.__name__, name)
    assert status("mx_conv_pack_weights_f16", None, 0, out(), out()) == ARG and status("mx_conv_pack_weights_f16", z, 0, None, out()) == ARG
    assert status("mx_conv_pack_weights_sp_f16", None, out(), out()) == ARG and status("mx_conv_pack_weights_sp_f16", z, out(), None) == ARG
    assert status("mx_conv_prep_fwd_f16", None, z, z, 1, 2, 8, out(), out()) == ARG and status("mx_conv_prep_fwd_f16", z, z, z, 1, 2, 353, out(), out()) == ARG
    assert status("mx_conv_prep_gpool_cl_f16", z, z, z, 1, 2, 8, out(), out(), None, None) == ARG         # g_idx is required, gidx is not
    assert status("mx_conv_prep_gpool_cl_f16", z, z, z, 1, 3, 8, out(), out(), out(), None) == ARG
    assert status("mx_ln_bwd_finish", z, z, z, None, 1, 64, 1, 8, out(), out(), out()) == ARG
    assert status("mx_ln_prelu_bwd_gpool_f16", z, z, z, z, z, None, z, 1, 1, 8, out(), out(), out(), None, out(), out(), out()) == ARG
    for o in outs:
        assert o.guards_intact() and o.untouched() == o.words

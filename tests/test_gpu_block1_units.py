"""GPU: the first block's f16x3 kernels and the head on their raw entry points, held to the independent fp64 references of
tests/helpers/block1_refs64.py -- mx_conv_prep_fwd_kvec_f16, mx_conv_pack_weights_kvec_f16, mx_conv_block1_fwd_f16,
mx_conv_block1_wgrad_f16, mx_conv_block1_wgrad_pair_f16, mx_ln_prelu_bwd_pair, mx_head_fwd, mx_head_bwd (conv_f16.hip,
wgrad_kvec_f16.hip, norm.hip, head_loss.hip).  Until now they were reached only through whole models, against fp32 torch at
1e-5 / 2e-5 of a tensor's maximum over seven layers.

Conventions of tests/test_gpu_general_units.py: every output lives between two guard bands pre-filled with a NaN bit pattern
that must survive; every launch has valid arguments; every tolerance gate is ``worst ratio to its bound <= tol``.
u = 2^-23 (one fp32 ulp of 1; an fp32 operation rounds by at most u / 2 of its result), gamma(n) = n u / (1 - n u).

* exact tests: operands are integers chosen so that every product and every partial sum is an integer below 2^24 (asserted from
  the fp64 sum of magnitudes): the fp32 accumulation of the matrix instructions is then exact in ANY order, and the result must
  equal the fp64 reference bit for bit -- one dropped split product, halo row, tile or unit shows;
* rounding tests: the project's 1e-5 of the tensor's maximum, and per element the split representation error 3 x 2^-22 plus
  gamma(number of accumulated terms + 2) of the sum of the magnitudes of the terms;
* f16x3 pairs: |hi + lo - v| <= 2^-22 |v| + 2^-25 (hi rounds by 2^-11 |v|, lo by 2^-11 of that, or by half the smallest fp16
  subnormal).
"""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests.helpers import block1_refs64 as R
from tests.helpers.general_refs64 import gamma
from tests.helpers.gpu_harness import (ARG, GUARD, POISON, SENT, U, UNSUPPORTED, Out, bits, bits16, call, dv, f16, f32, f64,  # noqa: F401
                                       normal16, pair_ok, ratio, relmax, status)

pytestmark = pytest.mark.gpu
P = R.PITCH


# ==== operand preparation ======================================================================================================
@pytest.mark.parametrize("H", [2, 6, 8, 10, 18])
@pytest.mark.parametrize("Wv", [1, 7, 345, 351, 352])
def test_prep_fwd_kvec(dev, H, Wv):
    """The statistics are GIVEN (fp64 mean / rstd rounded to fp32), so the kernel's only arithmetic is (x - mean) * rstd and the
    split.  H: below, at and off the 8 rows of a workgroup (2-row halo on each side); the pad columns of x hold 1e30."""
    g = np.random.default_rng(H * 1000 + Wv)
    B = 2
    x = np.full((B, 2, H, P), POISON, f32)
    x[..., :Wv] = (g.standard_normal((B, 2, H, Wv)) * 2.0 + 0.5).astype(f32)
    stats = R.plane_stats(x[..., :Wv]).astype(f32)
    hi_o, lo_o = Out(dev, B * H * P * 16, f16), Out(dev, B * H * P * 16, f16)
    call("mx_conv_prep_fwd_kvec_f16", dv(dev, x), dv(dev, stats), B, H, Wv, hi_o, lo_o)
    hi, lo = hi_o.read().reshape(B, H, P, 16), lo_o.read().reshape(B, H, P, 16)
    assert hi_o.guards_intact() and lo_o.guards_intact()
    zero = R.kvec_layout(np.ones((B, 2, H, Wv)), Wv) == 0
    assert not bits16(hi)[zero].any() and not bits16(lo)[zero].any()       # exact +0 wherever the layout says zero
    m32, r32 = stats[:, :, 0, None, None], stats[:, :, 1, None, None]
    v32 = R.kvec_layout((x[..., :Wv] - m32) * r32, Wv)                      # the same two fp32 operations
    ok = normal16(v32)
    assert ok.sum() > 0.9 * (~zero).sum()
    assert np.array_equal(bits16(hi)[ok], bits16(v32.astype(f16))[ok])
    v64 = R.kvec_layout(R.normalise(x[..., :Wv], stats), Wv)
    mag = R.kvec_layout((np.abs(x[..., :Wv].astype(f64)) + np.abs(m32.astype(f64))) * r32.astype(f64), Wv)
    tol = 1.0
    assert pair_ok(hi, lo, v64, 2 * U * mag) <= tol                        # fp32 operations of the formula: 2 (subtract, multiply)


def test_pack_weights_kvec(dev):
    g = np.random.default_rng(3)
    W = (g.standard_normal((64, 2, 5, 13)) / np.sqrt(130)).astype(f32)
    W[0, 0, 0, 0], W[1, 1, 4, 12] = 0.0, f32(2.0 ** -30)                     # an exact zero; W * 256 below the fp16 normal range
    hi_o, lo_o = Out(dev, 13 * 2 * 64 * 8, f16), Out(dev, 13 * 2 * 64 * 8, f16)
    call("mx_conv_pack_weights_kvec_f16", dv(dev, W), hi_o, lo_o)
    hi, lo = hi_o.read().reshape(13, 2, 64, 8), lo_o.read().reshape(13, 2, 64, 8)
    assert hi_o.guards_intact() and lo_o.guards_intact()
    v64 = R.kvec_weights(W)
    zero = R.kvec_weights(np.ones((64, 2, 5, 13))) == 0
    assert zero.sum() == 13 * 64 * 6 and not bits16(hi)[zero].any() and not bits16(lo)[zero].any()
    ok = normal16(v64)
    assert np.array_equal(bits16(hi)[ok], bits16(v64.astype(f32).astype(f16))[ok])     # W * 256 is exact in fp32
    tol = 1.0
    assert pair_ok(hi, lo, v64) <= tol                                     # fp32 operations of the formula: 0 (a power of two)


# ==== forward, exact ===========================================================================================================
def _schedule(B, H):
    """(tiles per workgroup, grid) by the entry point's own formula."""
    n = B * (H // 2)
    grid = min(1024, n)
    per = -(-n // grid)
    return per, -(-n // per)


_FWD_EXACT = {
    # name: (B, H, Wv, tiles per workgroup, grid, renumbering taken, last workgroup short)
    "1x2x17": (1, 2, 17, 1, 1, False, False), "2x6x345": (2, 6, 345, 1, 6, False, False), "3x8x351": (3, 8, 351, 1, 12, False, False),
    "2x10x352": (2, 10, 352, 1, 10, False, False), "1x4x1": (1, 4, 1, 1, 2, False, False),
    "tiles1025_2_per_wg_odd_grid_short_tail": (41, 50, 40, 2, 513, False, True),
    "tiles1040_grid520_renumbered": (40, 52, 40, 2, 520, True, False),
    "tiles2054_3_per_wg": (79, 52, 40, 3, 685, False, True),
}


def _exact_fwd_problem(B, H, Wv, seed):
    g = np.random.default_rng(seed)
    xh = 64.0 * g.integers(-4, 5, (B, 2, H, Wv))
    xl = g.integers(-8, 9, (B, 2, H, Wv)).astype(f64)
    if B > 1:                                                                # last clip: every row alike -> interior row pairs TIE
        xh[B - 1], xl[B - 1] = xh[B - 1, :, :1], xl[B - 1, :, :1]
    wh = 64.0 * g.integers(-4, 5, (64, 2, 5, 13))
    wl = g.integers(-8, 9, (64, 2, 5, 13)).astype(f64)
    bias = g.integers(-1024, 1025, 64) / 256.0
    # every partial sum is an integer below 2^24: sum over the 130 taps of the magnitudes of the three products + 256 |bias|
    worst = (np.abs(wh) + np.abs(wl)).sum((1, 2, 3)) * np.abs(xh).max() + np.abs(wh).sum((1, 2, 3)) * np.abs(xl).max() + 256 * np.abs(bias)
    assert worst.max() < 2.0 ** 24
    acc = R.conv1(xh, wh + wl) + R.conv1(xl, wh)                             # hi hi + hi lo + lo hi; lo lo is dropped by design
    pooled, amax = R.pool21(acc)
    out = pooled / 256.0 + bias[None, :, None, None]
    assert np.array_equal(out, out.astype(f32).astype(f64))
    return dict(xk_hi=R.kvec_layout(xh, Wv).astype(f16), xk_lo=R.kvec_layout(xl, Wv).astype(f16), w_hi=R.kvec_weights(wh, 1.0).astype(f16),
                w_lo=R.kvec_weights(wl, 1.0).astype(f16), bias=bias.astype(f32), out=out.astype(f32), amax=amax,
                ties=int((acc[:, :, 1::2] == acc[:, :, 0::2]).sum()))


@pytest.mark.parametrize("name", list(_FWD_EXACT))
def test_block1_fwd_exact_on_integers(dev, name):
    """x_hi = 64 a, x_lo = b, w_hi = 64 c, w_lo = d (|a|, |c| <= 4, |b|, |d| <= 8), bias a multiple of 1 / 256: out must equal
    (sum hi hi + hi lo + lo hi) / 256 + bias bit for bit and the argmax plane exactly (ties: the even row), with and without
    the optional statistics.  The schedule cases run the persistent kernel's multi-tile loop (LDS-DMA double buffering, a
    short last workgroup, tile ranges crossing clips) and its workgroup renumbering at Wv = 40."""
    B, H, Wv, per, grid, renum, short = _FWD_EXACT[name]
    assert _schedule(B, H) == (per, grid) and ((grid & 7) == 0) == renum and (per * grid > B * (H // 2)) == short
    pr = _exact_fwd_problem(B, H, Wv, 17 * B + H + Wv)
    assert pr["ties"] > 0 or H < 6 or B == 1
    Hp = H // 2
    n = B * 64 * Hp * P
    ops = [dv(dev, pr[k], f16) for k in ("xk_hi", "xk_lo", "w_hi", "w_lo")] + [dv(dev, pr["bias"])]
    slope = np.random.default_rng(1).uniform(0.05, 0.5, 64).astype(f32)
    out_s, am_s, sp = Out(dev, n), Out(dev, n, np.uint8), Out(dev, B * Hp * 64 * 2)
    call("mx_conv_block1_fwd_f16", *ops, B, H, Wv, out_s, am_s, dv(dev, slope), sp)
    out_n, am_n = Out(dev, n), Out(dev, n, np.uint8)
    call("mx_conv_block1_fwd_f16", *ops, B, H, Wv, out_n, am_n, None, None)
    for o in (out_s, am_s, sp, out_n, am_n):
        assert o.guards_intact()
    assert torch.equal(out_s.body_words(), out_n.body_words()) and torch.equal(am_s.body_words(), am_n.body_words())
    got = out_s.dev(torch.float32).view(B, 64, Hp, P)
    assert not bool(got[..., Wv:].view(torch.int32).any())                   # pad columns: written as +0
    want = torch.from_numpy(pr["out"]).to(dev)
    bad = (got[..., :Wv].contiguous().view(torch.int32) != want.view(torch.int32))
    assert not bool(bad.any()), (int(bad.sum()), got[..., :Wv][bad][:4].tolist(), want[bad][:4].tolist())
    gam = am_s.dev(torch.uint8).view(B, 64, Hp, P)[..., :Wv]
    assert bool((gam == torch.from_numpy(pr["amax"]).to(dev)).all())
    # the optional by-product: row sums of PReLU(out) - PReLU(bias) and of its square over w < Wv
    ref, mag = R.stats_rows(pr["out"], pr["bias"], slope)
    gsp = sp.read().reshape(B, Hp, 64, 2)
    tol = 1.0
    # Wv terms + 1, and per term the slope product, the shift's own product and the subtraction: gamma(Wv + 4);
    # squares: the error of d enters twice (2 x 3), the square rounds once: gamma(Wv + 8) of sum (|PReLU(out)| + |PReLU(bias)|)^2
    assert ratio(gsp[..., 0], ref[..., 0], gamma(Wv + 4) * mag[..., 0]) <= tol
    assert ratio(gsp[..., 1], ref[..., 1], gamma(Wv + 8) * mag[..., 1]) <= tol
    st = Out(dev, B * 64 * 2)
    call("mx_plane_stats_finish", sp, dv(dev, pr["bias"]), dv(dev, slope), B, 64, Hp, Wv, 1e-5, st)
    gst = st.read().reshape(B, 64, 2).astype(f64)
    assert st.guards_intact()
    y = R.prelu(pr["out"].astype(f64), slope.astype(f64)[None, :, None, None])
    mean_r, var_r = y.mean((2, 3)), y.var((2, 3))
    # the measures and gates of test_block_f16x3_kernels: the mean against the plane's standard deviation, rstd relatively.
    # They presume what holds for that test's planes: a second moment of d = PReLU(out) - PReLU(bias) of the order of the
    # variance.  var = E[d^2] - E[d]^2 from fp32 squares carries u / 2 of E[d^2], i.e. kappa = E[d^2] / var times that much
    # of var, whatever the kernel does; these integer planes have up to 2 elements a plane (Wv = 1), where kappa has no
    # bound.  The gates are held on the planes with kappa <= 16 (2e-6 = 34 u / 2), which must be most of them.
    d = y - R.prelu(pr["bias"].astype(f64), slope.astype(f64))[None, :, None, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        well = (d * d).mean((2, 3)) / var_r <= 16.0
    assert well.mean() > 0.5
    assert float((np.abs(gst[..., 0] - mean_r)[well] / np.sqrt(var_r[well])).max()) < 2e-6
    assert float(np.abs(gst[..., 1] * np.sqrt(var_r + 1e-5) - 1)[well].max()) < 2e-6


# ==== forward, rounding ========================================================================================================
@pytest.mark.parametrize("B,H,Wv", [(2, 16, 345), (2, 6, 88)])
def test_block1_fwd_rounding_on_random_floats(dev, B, H, Wv):
    """prep + pack + conv on random floats against the fp64 reference on the same fp32 inputs."""
    g = np.random.default_rng(H + Wv)
    x = np.zeros((B, 2, H, P), f32)
    x[..., :Wv] = (g.standard_normal((B, 2, H, Wv)) * 2.0 + 0.5).astype(f32)
    W = (g.standard_normal((64, 2, 5, 13)) / np.sqrt(130)).astype(f32)
    bias = (g.standard_normal(64) * 0.1).astype(f32)
    stats = R.plane_stats(x[..., :Wv]).astype(f32)
    xk = [Out(dev, B * H * P * 16, f16) for _ in range(2)]
    wk = [Out(dev, 13 * 2 * 64 * 8, f16) for _ in range(2)]
    call("mx_conv_prep_fwd_kvec_f16", dv(dev, x), dv(dev, stats), B, H, Wv, *xk)
    call("mx_conv_pack_weights_kvec_f16", dv(dev, W), *wk)
    n = B * 64 * (H // 2) * P
    out, am = Out(dev, n), Out(dev, n, np.uint8)
    call("mx_conv_block1_fwd_f16", *xk, *wk, dv(dev, bias), B, H, Wv, out, am, None, None)
    got = out.read().reshape(B, 64, H // 2, P)
    assert out.guards_intact() and am.guards_intact() and not bits(got[..., Wv:]).any()
    xhat = R.normalise(x[..., :Wv], stats)
    ref, _, z = R.conv1_pool_fwd(xhat, W, bias)
    zmag = R.conv1(np.abs(xhat), np.abs(W.astype(f64)))
    mag = np.maximum(zmag[:, :, 0::2], zmag[:, :, 1::2])
    assert relmax(got[..., :Wv], ref) < 1e-5
    tol = 1.0
    # the pairs represent W and xhat to 2^-22 each and drop lo lo (2^-22): 3 x 2^-22; 390 products and the bias in any order
    bound = (3 * 2.0 ** -22 + gamma(392)) * mag + U * np.abs(bias.astype(f64))[None, :, None, None]
    assert ratio(got[..., :Wv], ref, bound) <= tol
    # the argmax may differ from the reference's only where the two rows are closer than their bounds
    gam = am.read().reshape(B, 64, H // 2, P)[..., :Wv]
    diff = gam != (z[:, :, 1::2] > z[:, :, 0::2])
    assert (np.abs(z[:, :, 1::2] - z[:, :, 0::2])[diff] <= 2 * (3 * 2.0 ** -22 + gamma(392)) * mag[diff]).all()


# ==== weight gradient ==========================================================================================================
N_PART = 13 * 64 * 16                          # floats of one slab's partial result


def _wgrad_run(dev, entry, G_or_words, amax, third, xk_hi, xk_lo, B, H, Wv, rps):
    """One call with the workspace sized for the CALLER's rows_per_slab; returns (dW, scale or None) after the guard checks."""
    n_alloc = -(-(B * H) // rps)
    n_used = -(-(B * H) // (rps + (rps & 1)))
    part, dW = Out(dev, n_alloc * N_PART), Out(dev, 64 * 2 * 5 * 13)
    if entry == "mx_conv_block1_wgrad_f16":
        scale = Out(dev, 2)
        call(entry, G_or_words, amax, third, xk_hi, xk_lo, B, H, Wv, rps, scale, part, dW)
    else:
        scale = None
        call(entry, G_or_words, amax, third, xk_hi, xk_lo, B, H, Wv, rps, part, dW)
    got = dW.read().reshape(64, 2, 5, 13)
    assert part.guards_intact() and dW.guards_intact() and (scale is None or scale.guards_intact())
    assert part.untouched(n_used * N_PART) == (n_alloc - n_used) * N_PART, "a slab beyond those the call uses was written"
    assert part.untouched() == (n_alloc - n_used) * N_PART and dW.untouched() == 0
    return got, None if scale is None else scale.read()


@functools.lru_cache(maxsize=None)
def _exact_wgrad_problem(B, H, Wv):
    g = np.random.default_rng(B * 1000 + H * 100 + Wv)
    Hp = H // 2
    xh = 64.0 * g.integers(-4, 5, (B, 2, H, Wv))
    xl = g.integers(-8, 9, (B, 2, H, Wv)).astype(f64)
    Gv = g.integers(-3, 4, (B, 64, Hp, Wv)).astype(f64)
    Gv[B - 1, 63, Hp - 1, Wv - 1] = 768.0                                     # max |G| = 768 = 0.75 x 2^10: S = 2^0
    amax = g.integers(0, 2, (B, 64, Hp, P)).astype(np.uint8)
    av = amax[..., :Wv]
    G = np.full((B, 64, Hp, P), POISON, f32)                                  # fp32 entry: the pad columns are masked by Wv
    G[..., :Wv] = Gv
    # pair entry: scale = {4, 1 / 4}; hi + lo = 4 G with lo != 0 (except on the planted maximum: 3072 - lo is no fp16 number)
    lo = g.integers(-2, 3, (B, 64, Hp, Wv)).astype(f64)
    lo[B - 1, 63, Hp - 1, Wv - 1] = 0.0
    hi = 4.0 * Gv - lo
    words = np.zeros((B, 64, Hp, P), np.uint32)                              # the pad columns are zero words, as the contract says
    words[..., :Wv] = R.pack_pair(hi.astype(f16), lo.astype(f16))
    assert np.array_equal(hi.astype(f16).astype(f64), hi) and (lo != 0).mean() > 0.5
    ref = R.conv1_wgrad(R.route(Gv, av), xh + xl)
    # the pair entry multiplies hi (xh + xl) + lo xh: the same sum without the lo xl product, which f16x3 drops by design
    ref_pair = ref - R.conv1_wgrad(R.route(lo, av), xl) / 4.0
    # every slab's partial sums are integers below 2^24: bounded by the sum of the magnitudes over the WHOLE problem
    worst = R.conv1_wgrad(R.route(np.abs(hi) + np.abs(lo), av), np.abs(xh) + np.abs(xl)).max()
    assert worst < 2.0 ** 24
    assert np.array_equal(ref, ref.astype(f32).astype(f64)) and np.array_equal(ref_pair, ref_pair.astype(f32).astype(f64))
    pr = dict(G=G, Gv=Gv, amax=amax, words=words, xk_hi=R.kvec_layout(xh, Wv).astype(f16), xk_lo=R.kvec_layout(xl, Wv).astype(f16),
              ref=ref.astype(f32), ref_pair=ref_pair.astype(f32), ref64=ref)
    for a in pr.values():
        a.setflags(write=False)
    return pr


_WG_SHAPES = [(1, 2, 17), (5, 4, 345), (3, 6, 352), (2, 10, 200)]


@pytest.mark.parametrize("B,H,Wv", _WG_SHAPES)
def test_block1_wgrad_exact_on_integers(dev, B, H, Wv):
    """Integer operands, every slab sum exact: dW of both entry points must equal the fp64 reference rounded once to fp32 bit
    for bit, for every rows_per_slab -- odd ones (rounded up to whole pooling pairs by the entry point), slabs that straddle
    clips ((5, 4) with 6), a short last slab, one slab for everything; Wv = 200 ends inside the second chunk of a row."""
    pr = _exact_wgrad_problem(B, H, Wv)
    xk_hi, xk_lo, amax = dv(dev, pr["xk_hi"], f16), dv(dev, pr["xk_lo"], f16), dv(dev, pr["amax"], np.uint8)
    G, words = dv(dev, pr["G"]), dv(dev, pr["words"], np.uint32)
    amax_bits = dv(dev, np.array([768.0], f32))
    pair_scale = dv(dev, np.array([4.0, 0.25], f32))
    for rps in (1, 2, 3, 6, 16, B * H):
        got, scale = _wgrad_run(dev, "mx_conv_block1_wgrad_f16", G, amax, amax_bits, xk_hi, xk_lo, B, H, Wv, rps)
        assert scale.tolist() == [1.0, 1.0]
        bad = np.flatnonzero(bits(got) != bits(pr["ref"]))
        assert bad.size == 0, ("fp32 entry", rps, bad[:5], got.ravel()[bad[:5]], pr["ref"].ravel()[bad[:5]])
        got, _ = _wgrad_run(dev, "mx_conv_block1_wgrad_pair_f16", words, amax, pair_scale, xk_hi, xk_lo, B, H, Wv, rps)
        bad = np.flatnonzero(bits(got) != bits(pr["ref_pair"]))
        assert bad.size == 0, ("pair entry", rps, bad[:5], got.ravel()[bad[:5]], pr["ref_pair"].ravel()[bad[:5]])


def test_block1_wgrad_zero_and_scaled_gradients(dev):
    """An all-zero G (max |G| = 0) gives an all-zero finite dW; G x 2^+-40 with amax_bits to match gives dW x 2^+-40 exactly
    (S = 2^-+40: G S, hence every matrix product, is unchanged)."""
    B, H, Wv, rps = 3, 6, 352, 2
    pr = _exact_wgrad_problem(B, H, Wv)
    xk_hi, xk_lo, amax = dv(dev, pr["xk_hi"], f16), dv(dev, pr["xk_lo"], f16), dv(dev, pr["amax"], np.uint8)
    got, scale = _wgrad_run(dev, "mx_conv_block1_wgrad_f16", dv(dev, np.zeros_like(pr["G"])), amax, dv(dev, np.zeros(1, f32)), xk_hi, xk_lo,
                            B, H, Wv, rps)
    assert not got.any() and np.isfinite(got).all() and np.isfinite(scale).all()
    for e in (40, -40):
        got, scale = _wgrad_run(dev, "mx_conv_block1_wgrad_f16", dv(dev, pr["Gv"] * 2.0 ** e), amax, dv(dev, np.array([768.0 * 2.0 ** e], f32)),
                                xk_hi, xk_lo, B, H, Wv, rps)
        assert scale.tolist() == [2.0 ** -e, 2.0 ** e]
        assert np.array_equal(bits(got), bits((pr["ref64"] * 2.0 ** e).astype(f32))), e


def _pow2_scale(m):
    """The entry point's S: the power of two with m S in [512, 1024)."""
    return 2.0 ** (10 - int(np.frexp(f32(m))[1]))


def _wgrad_bound(dzmag, rps, Wv):
    """(3 x 2^-22 + gamma(3 x positions per slab + 2)) sum |dz| |xhat|: three matrix-instruction passes over the rows_per_slab x Wv
    positions of a slab in any order, the fp64 sum over the slabs and the final product, each rounded once."""
    return (3 * 2.0 ** -22 + gamma(3 * rps * Wv + 2)) * dzmag


def test_block1_wgrad_rounding_on_random_floats(dev):
    B, H, Wv, rps = 3, 8, 345, 6
    g = np.random.default_rng(21)
    Hp = H // 2
    xhat = (g.standard_normal((B, 2, H, Wv))).astype(f32)
    hi, lo = R.split16(R.kvec_layout(xhat, Wv))
    Gv = (g.standard_normal((B, 64, Hp, Wv)) * 1e-3).astype(f32)
    amax = g.integers(0, 2, (B, 64, Hp, P)).astype(np.uint8)
    G = np.full((B, 64, Hp, P), POISON, f32)
    G[..., :Wv] = Gv
    gmax = np.abs(Gv).max()
    S = _pow2_scale(gmax)
    words = np.zeros((B, 64, Hp, P), np.uint32)
    words[..., :Wv] = R.pack_pair(*R.split16(Gv * f32(S)))
    dz = R.route(Gv, amax[..., :Wv])
    ref = R.conv1_wgrad(dz, xhat)
    bound = _wgrad_bound(R.conv1_wgrad(np.abs(dz), np.abs(xhat)), rps, Wv)
    xk_hi, xk_lo, am = dv(dev, hi, f16), dv(dev, lo, f16), dv(dev, amax, np.uint8)
    got, scale = _wgrad_run(dev, "mx_conv_block1_wgrad_f16", dv(dev, G), am, dv(dev, np.array([gmax], f32)), xk_hi, xk_lo, B, H, Wv, rps)
    assert scale.tolist() == [S, 1.0 / S] and 512.0 <= gmax * S < 1024.0
    tol = 1.0
    assert relmax(got, ref) < 1e-5
    assert ratio(got, ref, bound) <= tol
    got, _ = _wgrad_run(dev, "mx_conv_block1_wgrad_pair_f16", dv(dev, words, np.uint32), am, dv(dev, np.array([S, 1.0 / S], f32)), xk_hi,
                        xk_lo, B, H, Wv, rps)
    assert relmax(got, ref) < 1e-5
    assert ratio(got, ref, bound) <= tol


# ==== LayerNorm + PReLU backward that leaves f16x3 pairs ===============================================================================
def _ln_problem(B, H, Wv, seed):
    g = np.random.default_rng(seed)
    C = 64
    p, d = np.full((B, C, H, P), POISON, f32), np.full((B, C, H, P), POISON, f32)
    p[..., :Wv] = g.standard_normal((B, C, H, Wv)).astype(f32)
    p[:, :, 0, 0], p[:, 1::2, H - 1, Wv - 1] = 0.0, -0.0                       # the kink: the slope branch
    d[..., :Wv] = (g.standard_normal((B, C, H, Wv)) * 1e-2).astype(f32)
    slope = g.uniform(0.05, 0.5, C).astype(f32)
    pv, dvv = p[..., :Wv], d[..., :Wv]
    stats = R.plane_stats(R.prelu(pv.astype(f64), slope.astype(f64)[None, :, None, None])).astype(f32)
    xh = R.ln_prelu_bwd(pv, dvv, stats, slope)["xhat"]
    halves = [slice(0, min(192, Wv)), slice(min(192, Wv), Wv)]                   # the producer's two position halves
    ln_part = np.stack([np.stack([dvv[..., s].astype(f64).sum(-1), (dvv[..., s] * xh[..., s]).sum(-1)], -1) for s in halves], -2).astype(f32)
    n = H * Wv
    m12 = (ln_part.astype(f64)[..., 0].sum((2, 3)) / n, ln_part.astype(f64)[..., 1].sum((2, 3)) / n)
    return dict(p=p, d=d, slope=slope, stats=stats, ln_part=ln_part, ref=R.ln_prelu_bwd(pv, dvv, stats, slope, m12=m12), xhat=xh)


@pytest.mark.parametrize("B,H,Wv", [(2, 4, 345), (1, 2, 17)])
def test_ln_prelu_bwd_pair(dev, B, H, Wv):
    """ln_part: fp64 sums rounded to fp32; scale: a chosen power of two.  The unpacked (hi + lo) / S is the G that
    mx_ln_prelu_bwd writes from the same inputs to 2^-22 |G| + 2^-25 / S; the pad columns are zero words; the per-plane sums
    are bit-identical; G is within the elementwise bound of the fp64 reference."""
    C = 64
    pr = _ln_problem(B, H, Wv, 31 * B + H + Wv)
    ref = pr["ref"]
    S = _pow2_scale(np.abs(ref["G"]).max())
    p, stats, slope, ln_part = dv(dev, pr["p"]), dv(dev, pr["stats"]), dv(dev, pr["slope"]), dv(dev, pr["ln_part"])
    n = B * C * H * P
    g_a, ds_a, gs_a = Out(dev, n, init=pr["d"]), Out(dev, B * C), Out(dev, B * C)
    g_b, ds_b, gs_b = Out(dev, n, init=pr["d"]), Out(dev, B * C), Out(dev, B * C)
    call("mx_ln_prelu_bwd", p, g_a, stats, slope, B, C, H, Wv, ds_a, gs_a, None, ln_part)
    call("mx_ln_prelu_bwd_pair", p, g_b, stats, slope, B, C, H, Wv, ds_b, gs_b, ln_part, dv(dev, np.array([S, 1.0 / S], f32)))
    for o in (g_a, ds_a, gs_a, g_b, ds_b, gs_b):
        assert o.guards_intact()
    Ga, words = g_a.read().reshape(B, C, H, P), g_b.read().view(np.uint32).reshape(B, C, H, P)
    assert not bits(Ga[..., Wv:]).any() and not words[..., Wv:].any()           # pad columns: zeros / zero words
    assert np.array_equal(bits(ds_a.read()), bits(ds_b.read())) and np.array_equal(bits(gs_a.read()), bits(gs_b.read()))
    hi, lo = R.unpack_pair(words[..., :Wv])
    tol = 1.0
    assert pair_ok(hi, lo, Ga[..., :Wv].astype(f64) * S) <= tol                 # G * S is exact in fp32: no operation beyond the split
    # fp32 operations of the formula: 10 (slope p, - mean, rstd; xhat m2, - m1, - , rstd, slope; the roundings of m1 and m2)
    assert ratio(Ga[..., :Wv], ref["G"], 10 * U * ref["G_mag"]) <= tol
    assert ratio((hi.astype(f64) + lo.astype(f64)) / S, ref["G"], 10 * U * ref["G_mag"] + 2.0 ** -22 * np.abs(ref["G"]) + 2.0 ** -25 / S) <= tol
    # per-plane sums kept in fp64 and rounded once; their terms carry the elementwise error above (10), one more product and the
    # 3 fp32 additions of a 4-element group: 14
    assert ratio(ds_a.read().reshape(B, C), ref["dslope"], U * np.abs(ref["dslope"]) + 14 * U * ref["dslope_mag"]) <= tol
    assert ratio(gs_a.read().reshape(B, C), ref["gsum"], U * np.abs(ref["gsum"]) + 14 * U * ref["gsum_mag"]) <= tol


def test_ln_bwd_finish_pair_wgrad_chain(dev):
    """mx_ln_bwd_finish -> mx_ln_prelu_bwd_pair -> mx_conv_block1_wgrad_pair_f16 as models.py chains them, against the fp64 dW."""
    B, Hp, Wv, C, rps = 2, 4, 345, 64, 1
    H = 2 * Hp
    pr = _ln_problem(B, Hp, Wv, 77)
    ref = pr["ref"]
    g = np.random.default_rng(78)
    xhat0 = g.standard_normal((B, 2, H, Wv)).astype(f32)                        # the first block's normalised input
    hi, lo = R.split16(R.kvec_layout(xhat0, Wv))
    amax = g.integers(0, 2, (B, C, Hp, P)).astype(np.uint8)
    gx = np.array([np.abs(pr["d"][..., :Wv]).max(), np.abs(pr["xhat"]).max()], f32)
    p, stats, slope, ln_part = dv(dev, pr["p"]), dv(dev, pr["stats"]), dv(dev, pr["slope"]), dv(dev, pr["ln_part"])
    m12, bound_ws, scale = Out(dev, B * C * 2), Out(dev, 1, np.uint32), Out(dev, 2)
    call("mx_ln_bwd_finish", ln_part, stats, slope, dv(dev, gx), B, C, Hp, Wv, m12, bound_ws, scale)
    S, inv = scale.read().tolist()
    gmax = float(np.abs(ref["G"]).max())
    assert m12.guards_intact() and scale.guards_intact() and bound_ws.guards_intact()
    assert S == 2.0 ** round(np.log2(S)) and inv == 1.0 / S and gmax * S < 1024.0   # a power of two from a true bound on max |G|
    words, ds, gs = Out(dev, B * C * Hp * P, init=pr["d"]), Out(dev, B * C), Out(dev, B * C)
    call("mx_ln_prelu_bwd_pair", p, words, stats, slope, B, C, Hp, Wv, ds, gs, ln_part, scale)
    assert words.guards_intact()
    got, _ = _wgrad_run(dev, "mx_conv_block1_wgrad_pair_f16", words, dv(dev, amax, np.uint8), scale, dv(dev, hi, f16), dv(dev, lo, f16),
                        B, H, Wv, rps)
    dz, dzmag = R.route(ref["G"], amax[..., :Wv]), R.route(ref["G_mag"], amax[..., :Wv])
    want = R.conv1_wgrad(dz, xhat0)
    # the weight gradient's own bound on sum |dz| |xhat|, plus G's elementwise error (10 u of its terms) carried through the sum
    bound = _wgrad_bound(R.conv1_wgrad(np.abs(dz), np.abs(xhat0)), rps + 1, Wv) + 10 * U * R.conv1_wgrad(dzmag, np.abs(xhat0))
    tol = 1.0
    assert relmax(got, want) < 1e-5
    assert ratio(got, want, bound) <= tol


# ==== head =====================================================================================================================
def _pairwise(levels):
    """A greedy pairwise-covering subset of the full product (deterministic)."""
    names = list(levels)
    need = {(i, a, j, b) for i, j in itertools.combinations(range(len(names)), 2) for a in levels[names[i]] for b in levels[names[j]]}
    full, picked = list(itertools.product(*levels.values())), []
    while need:
        cover = lambda c: {(i, c[i], j, c[j]) for i, j in itertools.combinations(range(len(names)), 2)} & need
        best = max(full, key=lambda c: len(cover(c)))
        need -= cover(best)
        picked.append(best)
    return picked


_HEAD = _pairwise(dict(C=[64, 5, 3], Hl=[1, 4, 8], L=[1, 2, 4], Wv=[1, 63, 64, 65, 345, 352], B=[1, 3], dlat=[True, False]))


@pytest.mark.parametrize("C,Hl,L,Wv,B,dlat", _HEAD)
def test_head_fwd_bwd(dev, C, Hl, L, Wv, B, dlat):
    """C < 4 leaves channel groups of the forward kernel empty; p6 holds exact +0, -0 and values either side of the kink."""
    g = np.random.default_rng(C * 1000 + Hl * 100 + L * 10 + Wv + B)
    p6 = np.full((B, C, Hl, P), POISON, f32)
    v = g.standard_normal((B, C, Hl, Wv)).astype(f32)
    idx = np.arange(v.size).reshape(v.shape) % 11
    for r, val in enumerate((0.0, -0.0, 1e-30, -1e-30)):
        v[idx == r] = val
    p6[..., :Wv] = v
    slope = g.uniform(0.05, 0.5, C).astype(f32)
    k = 1 / np.sqrt(C)
    wout, bout = g.uniform(-k, k, (L, C)).astype(f32), g.uniform(-k, k, L).astype(f32)
    lat, out = Out(dev, B * C * Wv), Out(dev, B * L * Wv)
    call("mx_head_fwd", dv(dev, p6), dv(dev, slope), dv(dev, wout), dv(dev, bout), B, C, Hl, Wv, L, lat, out)
    glat, gout = lat.read().reshape(B, C, Wv), out.read().reshape(B, L, Wv)
    assert lat.guards_intact() and out.guards_intact() and lat.untouched() == 0 and out.untouched() == 0
    fr = R.head_fwd(v, slope, wout, bout)
    tol = 1.0
    # Hl terms, the slope product, 1 / Hl and the product with it: gamma(Hl + 3)
    assert ratio(glat, fr["latent"], gamma(Hl + 3) * fr["latent_mag"]) <= tol
    # the sigmoid on the latent the kernel wrote (gated above): C fused multiply-adds, 3 additions of the group partials and the
    # bias round the logit by (C + 4) u of its terms, of which the sigmoid (slope <= 1 / 4) passes a quarter; expf is documented
    # to 1 ulp, 1 + e and the division round once each: 4 u of 1 with the rounding of the argument
    f2 = R.head_fwd(np.broadcast_to(glat[:, :, None, :], (B, C, 1, Wv)), np.ones(C), wout, bout)
    assert ratio(gout, f2["out"], 4 * U + (C + 4) * U * f2["pre_mag"] / 4) <= tol
    # backward from inputs of its own: latent / out = the fp64 forward rounded to fp32
    lat_in, out_in = fr["latent"].astype(f32), fr["out"].astype(f32)
    d_out, d_lat = g.standard_normal((B, L, Wv)).astype(f32), g.standard_normal((B, C, Wv)).astype(f32) if dlat else None
    G6, dw, db, ds = Out(dev, B * C * Hl * P), Out(dev, B * L * C), Out(dev, B * L), Out(dev, B * C)
    gmax = torch.zeros(1, dtype=torch.int32, device=dev)
    call("mx_head_bwd", dv(dev, p6), dv(dev, slope), dv(dev, wout), dv(dev, lat_in), dv(dev, out_in), dv(dev, d_out),
         None if d_lat is None else dv(dev, d_lat), B, C, Hl, Wv, L, G6, dw, db, ds, gmax)
    gG, gdw, gdb, gds = G6.read().reshape(B, C, Hl, P), dw.read().reshape(B, L, C), db.read().reshape(B, L), ds.read().reshape(B, C)
    for o in (G6, dw, db, ds):
        assert o.guards_intact() and o.untouched() == 0
    assert not bits(gG[..., Wv:]).any()                                         # G6 is written as zeros on [Wv, 352)
    assert int(gmax.cpu()) == int(bits(np.abs(gG).max())[0])                        # the bit pattern of max |G6| of the returned tensor
    br = R.head_bwd(v, slope, wout, lat_in, out_in, d_out, d_lat)
    # d_out s (1 - s): 3; L fused multiply-adds onto d_latent; 1 / Hl and the product with it: 2; the slope: 1 -> L + 6
    assert ratio(gG[..., :Wv], br["G6"], (L + 6) * U * br["G6_mag"]) <= tol
    # per-clip partials: fp32 sums over w in any order; each term carries the 3 operations of dlogit (+ 1 product)
    assert ratio(gdb, br["dbout"], gamma(Wv + 4) * br["dbout_mag"]) <= tol
    assert ratio(gdw, br["dwout"], gamma(Wv + 5) * br["dwout_mag"]) <= tol
    assert ratio(gds, br["dslope"], gamma(Hl * Wv + L + 7) * br["dslope_mag"]) <= tol
    # ... which reduce over the clips to the parameter gradients (fp64 sums of the partials: the bounds add)
    assert ratio(gdw.astype(f64).sum(0), br["dwout"].sum(0), gamma(Wv + 5) * br["dwout_mag"].sum(0)) <= tol
    assert ratio(gdb.astype(f64).sum(0), br["dbout"].sum(0), gamma(Wv + 4) * br["dbout_mag"].sum(0)) <= tol
    assert ratio(gds.astype(f64).sum(0), br["dslope"].sum(0), gamma(Hl * Wv + L + 7) * br["dslope_mag"].sum(0)) <= tol


def test_documented_statuses_without_a_launch(dev):
    z = torch.zeros(1 << 16, device=dev)
    head_f = lambda p6=z, L=4, Wv=8: status("mx_head_fwd", p6, z, z, z, 1, 3, 2, Wv, L, z, z)
    head_b = lambda p6=z, L=4, Wv=8, G6=z: status("mx_head_bwd", p6, z, z, z, z, z, None, 1, 3, 2, Wv, L, G6, z, z, z, None)
    assert head_f(L=5) == UNSUPPORTED and head_b(L=5) == UNSUPPORTED
    assert head_f(Wv=353) == UNSUPPORTED and head_b(Wv=353) == UNSUPPORTED
    assert head_f(p6=None) == ARG and head_b(p6=None) == ARG and head_b(G6=None) == ARG
    fwd = lambda H=2, Wv=8, out=z: status("mx_conv_block1_fwd_f16", z, z, z, z, z, 1, H, Wv, out, z, None, None)
    wg = lambda H=2, Wv=8, dW=z: status("mx_conv_block1_wgrad_f16", z, z, z, z, z, 1, H, Wv, 2, z, z, dW)
    wgp = lambda H=2, Wv=8, dW=z: status("mx_conv_block1_wgrad_pair_f16", z, z, z, z, z, 1, H, Wv, 2, z, dW)
    for entry, last in ((fwd, "out"), (wg, "dW"), (wgp, "dW")):
        assert entry(H=3) == UNSUPPORTED and entry(Wv=353) == UNSUPPORTED and entry(**{last: None}) == ARG
    assert status("mx_conv_block1_fwd_f16", z, z, z, z, z, 1, 2, 8, z, z, None, z) == ARG      # stats_part without slope_out
    # the streaming preparation passes treat a width beyond the plane as a bad argument
    assert status("mx_conv_prep_fwd_kvec_f16", z, z, 1, 2, 353, z, z) == ARG
    assert status("mx_conv_prep_fwd_kvec_f16", None, z, 1, 2, 8, z, z) == ARG
    assert status("mx_conv_pack_weights_kvec_f16", None, z, z) == ARG
    assert status("mx_ln_prelu_bwd_pair", z, z, z, z, 1, 1, 1, 353, z, z, z, z) == ARG
    assert status("mx_ln_prelu_bwd_pair", z, z, z, z, 1, 1, 1, 8, z, z, None, z) == ARG         # ln_part is required

"""CPU: the references, layouts, bounds and the fp32 emulation of tests/helpers/f32block_refs64.py, which
tests/test_gpu_f32block_units.py holds the exact-fp32 conv block kernels to.

* the generic convolution references at Cin = 2 WITH a dilation against torch's fp64 autograd (tests/test_midblock_refs64.py and
  tests/test_block1_refs64.py hold Cin = 2 only undilated);
* the packed-weight and workspace layouts reproduce the convolution;
* the emulated fp32 arithmetic (fused multiply-adds in the natural and in the reversed tap order) is bit-exact on the integer
  problems and stays inside both gates on the float problems;
* test_defects_are_seen: every deliberate deviation fails the comparison the GPU test makes.
"""
import numpy as np
import pytest
import torch

from tests.helpers import f32block_refs64 as F

f32, f64 = np.float32, np.float64
bits = lambda a: np.ascontiguousarray(a, f32).view(np.int32)


def ratio(got, ref, bound):
    err = np.abs(np.asarray(got, f64) - np.asarray(ref, f64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / np.maximum(np.asarray(bound, f64), 1e-300))
    return float(np.max(r)) if r.size else 0.0


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ==== references and layouts =========================================================================================================
@pytest.mark.parametrize("T", [2, 16])
@pytest.mark.parametrize("Cin", [2, 4])
def test_generic_references_dilated_against_torch_fp64(Cin, T):
    """conv64 / conv64_dgrad / conv64_wgrad with few input channels and a dilation: torch.nn.functional.conv2d in fp64, dilation
    (1, T), padding (2, 6 T), and its autograd."""
    g = np.random.default_rng(Cin * 10 + T)
    B, H, Wd = 2, 4, 23
    x, W, dz = g.standard_normal((B, Cin, H, Wd)), g.standard_normal((64, Cin, 5, 13)), g.standard_normal((B, 64, H, Wd))
    xt, Wt = torch.tensor(x, requires_grad=True), torch.tensor(W, requires_grad=True)
    z = torch.nn.functional.conv2d(xt, Wt, dilation=(1, T), padding=(2, 6 * T))
    z.backward(torch.tensor(dz))
    tol = 1e-13
    assert rel(F.conv64(x, W, T), z.detach().numpy()) <= tol
    assert rel(F.conv64_dgrad(dz, W, T), xt.grad.numpy()) <= tol
    assert rel(F.conv64_wgrad(dz, x, T), Wt.grad.numpy()) <= tol
    # per-slab weight gradients add up to the whole, for slabs that cross a clip boundary and for one slab
    for rps in (1, 3, B * H + 5):
        parts = F.wgrad_parts(dz, x, T, B, H, rps)
        assert parts.shape[0] == -(-B * H // rps) and rel(parts.sum(0), Wt.grad.numpy()) <= tol


@pytest.mark.parametrize("Cout,Cin", [(64, 64), (64, 2), (5, 3)])
def test_layouts_reproduce_the_convolution(Cout, Cin):
    """flip 0: z = sum wt[ci][kh][kw][co] x[ci][h + kh - 2][w + (kw - 6) T]; flip 1: the SAME gather on dz with the roles of the
    channels exchanged gives the data gradient; the workspace layout is (slab, kh, kw, co, ci)."""
    g = np.random.default_rng(Cout + Cin)
    B, H, Wd, T = 1, 4, 9, 2
    W = g.standard_normal((Cout, Cin, 5, 13))
    x, dz = g.standard_normal((B, Cin, H, Wd)), g.standard_normal((B, Cout, H, Wd))

    def gather_conv(v, wt):                                                   # wt [c_in][kh][kw][c_out]
        vp = np.zeros((B, v.shape[1], H + 4, Wd + 12 * T))
        vp[:, :, 2:2 + H, 6 * T:6 * T + Wd] = v
        out = np.zeros((B, wt.shape[3], H, Wd))
        for kh in range(5):
            for kw in range(13):
                out += np.einsum("io,bihw->bohw", wt[:, kh, kw], vp[:, :, kh:kh + H, kw * T:kw * T + Wd])
        return out

    wt0, wt1 = F.pack_weights(W, 0), F.pack_weights(W, 1)
    assert wt0.shape == (Cin, 5, 13, Cout) and wt1.shape == (Cout, 5, 13, Cin)
    if Cout == 64:
        assert rel(gather_conv(x, wt0), F.conv64(x, W, T)) <= 1e-13
        assert rel(gather_conv(dz, wt1), F.conv64_dgrad(dz, W, T)) <= 1e-13
    for (co, ci, kh, kw) in ((0, 0, 0, 0), (Cout - 1, Cin - 1, 4, 12), (1, 2 % Cin, 3, 5)):
        assert wt0[ci, kh, kw, co] == W[co, ci, kh, kw] and wt1[co, 4 - kh, 12 - kw, ci] == W[co, ci, kh, kw]
    dWs = g.standard_normal((3, 64, Cin, 5, 13))
    assert F.part_layout(dWs)[2, 4, 12, 7, Cin - 1] == dWs[2, 7, Cin - 1, 4, 12]


def test_statistics_bound_holds_for_the_kernel_arithmetic():
    """fl32(slope x), fp64 sums, ss / n - mean^2, one rounding: inside stats_ref's bound, the constant plane and the planes with
    |mean| / std = 1e3 included; the fp32-rounded fp64 plane sum inside sum_ref's."""
    for (B, C, H, Wv, sl) in ((2, 1, 1, 1, True), (2, 3, 4, 17, True), (2, 3, 16, 352, True), (2, 3, 3, 345, False)):
        x, slope = F.stats_problem(B, C, H, Wv, sl)
        ref, bound = F.stats_ref(x, slope, Wv)
        xv = x[..., :Wv]
        t = xv if slope is None else np.where(xv > 0, xv, (slope[None, :, None, None] * xv).astype(f32))
        t = t.astype(f64)
        n = H * Wv
        mean = t.sum((2, 3)) / n
        var = np.maximum((t * t).sum((2, 3)) / n - mean * mean, 0.0)
        got = np.stack([mean, 1.0 / np.sqrt(var + F.EPS)], -1).astype(f32)
        assert ratio(got, ref, bound) <= 1.0
        assert ratio(got[0, 0, 1], 1.0 / np.sqrt(F.EPS), bound[0, 0, 1]) <= 1.0 and bound[0, 0, 1] < 1e-4
        s, sb = F.sum_ref(x, Wv)
        assert ratio(xv.astype(f64).sum((2, 3)).astype(f32), s, sb) <= 1.0


# ==== the emulated arithmetic ========================================================================================================
def _conv_sel(B, C, rows, Wv, n=48, seed=0):
    """Outputs (b, channel, row, w): the corners and edges of the image, and random ones."""
    g = np.random.default_rng(seed)
    b, c, h, w = g.integers(0, B, n), g.integers(0, C, n), g.integers(0, rows, n), g.integers(0, Wv, n)
    h[:8], w[:8] = [0, 0, rows - 1, rows - 1, 0, rows - 1, 0, rows - 1], [0, Wv - 1, 0, Wv - 1, Wv // 2, Wv // 2, min(5, Wv - 1), max(Wv - 6, 0)]
    return b, c, h, w


def _w_sel(Cin, n=32, seed=0):
    g = np.random.default_rng(seed)
    co, ci, kh, kw = g.integers(0, 64, n), g.integers(0, Cin, n), g.integers(0, 5, n), g.integers(0, 13, n)
    kh[:4], kw[:4] = [0, 4, 0, 4], [0, 12, 12, 0]
    return co, ci, kh, kw


def _float_runs(B, H, Wv, T, order, defect=None, cins=(2, 64), kinds=("fwd", "dgrad", "wgrad"), grads=F.GRAD_KINDS, rps=3):
    """Every float comparison of the GPU file on the emulated kernels: yields (name, ratio to Gate A, ratio to Gate B)."""
    for Cin in cins:
        p = F.float_problem(B, H, Wv, Cin)
        if "fwd" in kinds:
            ref, sel = F.float_fwd(B, H, Wv, Cin, T), _conv_sel(B, 64, H // 2, Wv)
            got, am = F.emulate("fwd", p, T, Wv, sel, order, defect)
            assert defect is not None or np.array_equal(am[ref["decided"][sel]], ref["amax"][sel][ref["decided"][sel]])
            yield f"fwd-{Cin}", ratio(got, ref["out"][sel], ref["bound"][sel]), ratio(got, ref["out"][sel], F.gate_b("fwd", ref["out"]))
        for kind in grads:
            gr = F.float_grads(B, H, Wv, kind)
            if "dgrad" in kinds and Cin == 64:
                ref, sel = F.float_dgrad(B, H, Wv, T, kind), _conv_sel(B, 64, H, Wv)
                got = F.emulate("dgrad", p, T, Wv, sel, order, defect, grads=gr)
                yield f"dgrad-{kind}", ratio(got, ref["dx"][sel], ref["bound"][sel]), ratio(got, ref["dx"][sel], F.gate_b("dgrad", ref["dx"]))
            if "wgrad" in kinds:
                ref, sel = F.float_wgrad(B, H, Wv, Cin, T, kind), _w_sel(Cin)
                got = F.emulate("wgrad", p, T, Wv, sel, order, defect, rows_per_slab=rps, grads=gr)
                yield f"wgrad-{Cin}-{kind}", ratio(got, ref["dW"][sel], ref["bound"][sel]), ratio(got, ref["dW"][sel], F.gate_b("wgrad", ref["dW"]))


@pytest.mark.parametrize("order", ["natural", "reversed"])
@pytest.mark.parametrize("T", [1, 16])
@pytest.mark.parametrize("B,H,Wv", F.ROUNDING_SHAPES)
def test_gates_hold_for_the_arithmetic(B, H, Wv, T, order):
    """fp32 arithmetic without a defect stays within the derived per-element bound (Gate A) and within the project's parity
    numbers against fp64 (Gate B), in both accumulation orders, one slab per three rows and one slab for the whole batch."""
    for rps in (3, B * H):
        for name, a, b in _float_runs(B, H, Wv, T, order, kinds=("fwd", "dgrad", "wgrad") if rps == 3 else ("wgrad",), rps=rps):
            assert a <= 1.0 and b <= 1.0, (name, rps, a, b)


def test_band_share_of_the_pooling_decisions():
    """From the reference alone: at most BAND_SHARE of the pooled elements have their two rows within BAND max |z|."""
    for (B, H, Wv) in F.ROUNDING_SHAPES:
        for Cin in (2, 64):
            for T in (1, 16):
                assert 1.0 - F.float_fwd(B, H, Wv, Cin, T)["decided"].mean() <= F.BAND_SHARE


# ==== teeth ==========================================================================================================================
_ALL = ("fwd", "dgrad", "wgrad")
_APPLIES = {"tie_takes_second": ("fwd",), "taps_not_mirrored": ("dgrad",), "stats_of_clip_0": ("fwd", "wgrad"),
            "slab_last_row_dropped": ("wgrad",), "prelu_skipped": ("fwd", "wgrad"), "route_ignores_amax": ("dgrad", "wgrad")}


def _exact_runs(B, H, Wv, Cin, T, order, defect, kinds, rps=5):
    """The exact comparisons of the GPU file on the emulated kernels: yields (name, number of selected outputs that differ)."""
    p = F.exact_problem(B, H, Wv, Cin)
    g = np.random.default_rng(1)
    if "fwd" in kinds:
        # all positions of four channels (one of them with tying edge pairs) of the last clip, whose interior pooling pairs tie
        chans = np.concatenate([[16], g.integers(0, 64, 3)])
        b, c, hp, ww = (a.ravel() for a in np.meshgrid([B - 1], chans, np.arange(H // 2), np.arange(Wv), indexing="ij"))
        ref = F.exact_fwd(B, H, Wv, Cin, T)
        assert ref["ties"] > 0
        got, am = F.emulate("fwd", p, T, Wv, (b, c, hp, ww), order, defect)
        yield "fwd", int((bits(got) != bits(ref["out"][b, c, hp, ww])).sum() + (am != ref["amax"][b, c, hp, ww]).sum())
    if "dgrad" in kinds and Cin == 64:
        sel = tuple(a.ravel() for a in np.meshgrid([0], [0, 41], np.arange(H), np.arange(Wv), indexing="ij"))
        got = F.emulate("dgrad", p, T, Wv, sel, order, defect, grads=p)
        yield "dgrad", int((bits(got) != bits(F.exact_dgrad(B, H, Wv, T)["dx"][sel])).sum())
    if "wgrad" in kinds:
        wsel = tuple(a.ravel() for a in np.meshgrid([3, 40], sorted({0, 9 % Cin, Cin - 1}), np.arange(5), np.arange(13), indexing="ij"))
        got = F.emulate("wgrad", p, T, Wv, wsel, order, defect, rows_per_slab=rps, grads=p)
        yield "wgrad", int((bits(got) != bits(F.exact_wgrad(B, H, Wv, Cin, T)["dW"][wsel])).sum())


@pytest.mark.parametrize("order", ["natural", "reversed"])
@pytest.mark.parametrize("Cin", [2, 4, 64])
def test_the_emulation_is_exact_on_the_integer_problems(Cin, order):
    """Without a defect the emulated kernels reproduce the fp64 references bit for bit in either order (dilations 1 and 16)."""
    for T in (1, 16):
        for name, n_bad in _exact_runs(2, 6, 17, Cin, T, order, None, _ALL if Cin != 4 else ("fwd",)):
            assert n_bad == 0, (T, name, n_bad)


@pytest.mark.parametrize("defect", F.DEFECTS)
def test_defects_are_seen(defect):
    """Each deliberate deviation fails the comparison the GPU test makes, for every kernel it can occur in: structural defects
    fail the exact comparison on the integer problem; operands truncated to a 10-bit mantissa leave small integers alone and
    fail Gate B on the float problem (Gate A, a worst-case bound, does not see them: that is why Gate B is there)."""
    B, H, Wv, T = 2, 6, 17, 2
    kinds = _APPLIES.get(defect, _ALL)
    if defect == "operands_truncated_to_tf32":
        assert all(n == 0 for _, n in _exact_runs(B, H, Wv, 64, T, "natural", defect, kinds))
        seen = {name: b for name, a, b in _float_runs(2, 4, 17, T, "natural", defect, grads=("gauss",))}
        assert {k.split("-")[0] for k in seen} == set(kinds) and all(b > 1.0 for b in seen.values()), seen
        return
    seen = dict(_exact_runs(B, H, Wv, 64, T, "natural", defect, kinds))
    assert set(seen) == set(kinds) and all(n > 0 for n in seen.values()), seen
    if defect not in ("prelu_skipped", "taps_not_mirrored"):                  # the first block (no slope; no data gradient)
        seen = dict(_exact_runs(B, H, Wv, 2, T, "natural", defect, [k for k in kinds if k != "dgrad"]))
        assert seen and all(n > 0 for n in seen.values()), seen

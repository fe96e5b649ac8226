"""CPU: the fp64 references of tests/helpers/midblock_refs64.py against torch's fp64 conv2d / max_pool2d / layer_norm / prelu
autograd to 1e-12 of the tensor's maximum, every operand layout against the convolution it must reproduce, the per-element
bounds of tests/test_gpu_midblock_units.py against a numpy emulation of the f16x3 arithmetic (if the arithmetic itself cannot
meet a bound, the bound is wrong, not the kernel), and that emulation with one deliberate defect at a time against the
comparisons the GPU tests make (a defect that no comparison sees means the tests have no teeth there)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import midblock_refs64 as M

f16, f32, f64 = np.float16, np.float32, np.float64
P = M.PITCH


def rel(got, ref):
    ref = np.asarray(ref, f64)
    return float(np.abs(np.asarray(got, f64) - ref).max() / max(float(np.abs(ref).max()), 1e-300))


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, f64))


# ==== references against torch ===================================================================================================
@pytest.mark.parametrize("T", M.DILATIONS)
@pytest.mark.parametrize("B,H,W", [(1, 2, 1), (2, 4, 17), (2, 6, 40)])
def test_block_forward_and_gradients(B, H, W, T):
    """Taps fall outside the image at every one of these shapes (W <= 6 T for all but (40, T <= 4))."""
    g = np.random.default_rng(B * 100 + H * 10 + W + T)
    p_prev = g.standard_normal((B, 64, H, W)) * 0.7 + 0.1
    slope = g.uniform(0.05, 0.45, 64)
    Wt, bias = g.standard_normal((64, 64, 5, 13)) / np.sqrt(4160), g.standard_normal(64) * 0.1
    Gc = g.standard_normal((B, 64, H // 2, W))
    y = M.prelu(p_prev, slope[None, :, None, None])
    stats = M.plane_stats(y)
    xhat = M.normalise(y, stats)
    out, amax, z = M.conv64_pool_fwd(xhat, Wt, bias, T)
    mag = M.conv64(np.abs(xhat), np.abs(Wt), T)
    dz = M.route(Gc, amax)
    dxhat, dW = M.conv64_dgrad(dz, Wt, T), M.conv64_wgrad(dz, xhat, T)
    ln = M.ln_prelu_bwd(p_prev, dxhat, stats, slope)

    p_t, s_t, w_t = t64(p_prev).requires_grad_(True), t64(slope).requires_grad_(True), t64(Wt).requires_grad_(True)
    xhat_t = F.layer_norm(F.prelu(p_t, s_t), (H, W), eps=1e-5)
    xhat_t.retain_grad()
    z_t = F.conv2d(xhat_t, w_t, t64(bias), dilation=(1, T), padding="same")
    o_t, idx = F.max_pool2d(z_t, (2, 1), return_indices=True)
    (o_t * t64(Gc)).sum().backward()
    tol = 1e-12
    assert rel(xhat, xhat_t.detach().numpy()) <= tol
    assert rel(z + bias[None, :, None, None], z_t.detach().numpy()) <= tol
    assert rel(out, o_t.detach().numpy()) <= tol
    assert rel(mag, F.conv2d(t64(np.abs(xhat)), t64(np.abs(Wt)), dilation=(1, T), padding="same").numpy()) <= tol
    assert (np.abs(z) <= mag * (1 + 1e-12)).all()
    rows = (idx.numpy() // W) % 2
    gap = np.abs(z[:, :, 1::2] - z[:, :, 0::2])
    assert np.array_equal(amax[gap > 1e-9], rows[gap > 1e-9].astype(np.uint8))
    assert rel(dxhat, xhat_t.grad.numpy()) <= tol
    assert rel(dW, w_t.grad.numpy()) <= tol
    assert rel(ln["G"], p_t.grad.numpy()) <= tol
    assert rel(ln["dslope"].sum(0), s_t.grad.numpy()) <= tol


def test_window_and_tap_sums():
    """The two cheap companions of the bounds equal the convolutions they abbreviate."""
    g = np.random.default_rng(3)
    B, H, W, T = 2, 4, 21, 4
    v, Wt = np.abs(g.standard_normal((B, 64, H, W))), np.abs(g.standard_normal((64, 64, 5, 13)))
    tol = 1e-12
    assert rel(M.window_sum(v.sum(1), T)[:, None] + 0 * v[:, :1], M.conv64(v, np.ones((1, 64, 5, 13)), T)) <= tol
    ones = np.ones((1, 64, H, W))
    assert rel(M.taps_inside(Wt.sum(1), H, W, T, False)[None], M.conv64(ones, Wt, T)) <= tol
    assert rel(M.taps_inside(Wt.sum(0), H, W, T, True)[None], M.conv64_dgrad(ones, Wt, T)) <= tol


# ==== layouts ====================================================================================================================
def _problem(T, seed=5, B=2, H=4, Wv=9):
    g = np.random.default_rng(seed + T)
    xhat, Wt = g.standard_normal((B, 64, H, Wv)), g.standard_normal((64, 64, 5, 13))
    G, amax = g.standard_normal((B, 64, H // 2, Wv)), g.integers(0, 2, (B, 64, H // 2, P)).astype(np.uint8)
    return B, H, Wv, xhat, Wt, G, amax


def _dense_contract(op, wp, H, Wv, T):
    """sum over (cb, kh, kw, khalf, j) of wp[cb][kh][kw][khalf][out][j] op[b][h + kh - 2][cb][w + (kw - 6) T][8 khalf + j]."""
    B = op.shape[0]
    opp = np.zeros((B, H + 4, 4, P + 12 * T, 16))
    opp[:, 2:2 + H, :, 6 * T:6 * T + P] = op
    w16 = wp.transpose(0, 1, 2, 4, 3, 5).reshape(4, 5, 13, 64, 16)          # [cb][kh][kw][out][16]
    return sum(np.einsum("bhcwk,cok->bohw", opp[:, kh:kh + H, :, kw * T:kw * T + Wv], w16[:, kh, kw])
               for kh in range(5) for kw in range(13))


@pytest.mark.parametrize("T", M.DILATIONS)
def test_dense_layouts_reproduce_the_convolution(T):
    """Contracting the packed weights with the channels-last operand over the documented indices gives 256 x the convolution
    (flip = 0) and 256 x its transpose (flip = 1); zeros exactly where the ABI says."""
    B, H, Wv, xhat, Wt, G, amax = _problem(T)
    wide = np.full((B, 64, H, Wv + 3), 1e30)                               # columns beyond Wv must not show
    wide[..., :Wv] = xhat
    op = M.cl_layout(wide, Wv)
    assert op.shape == (B, H, 4, P, 16) and not op[:, :, :, Wv:].any() and (op[:, :, :, :Wv] != 0).all()
    assert op[1, 2, 3, 4, 5] == xhat[1, 16 * 3 + 5, 2, 4] and np.array_equal(M.cl_planes(op)[..., :Wv], xhat)
    w0, w1 = M.pack_weights(Wt, 0), M.pack_weights(Wt, 1)
    assert w0.shape == (4, 5, 13, 2, 64, 8) and w0.size == M.W_ELEMS
    assert w0[2, 1, 3, 1, 7, 5] == 256 * Wt[7, 32 + 8 + 5, 1, 3] and w1[2, 1, 3, 1, 7, 5] == 256 * Wt[32 + 8 + 5, 7, 3, 9]
    tol = 1e-12
    assert rel(_dense_contract(op, w0, H, Wv, T) / 256, M.conv64(xhat, Wt, T)) <= tol
    dz = M.route(G, amax[..., :Wv])
    assert rel(_dense_contract(M.cl_layout(dz, Wv), w1, H, Wv, T) / 256, M.conv64_dgrad(dz, Wt, T)) <= tol


@pytest.mark.parametrize("T", M.DILATIONS)
def test_sparse_layouts_reproduce_the_gradients(T):
    """The pooled pair + g_idx words + fragment-ordered weights give 256 x the data gradient of the routed G; the pooled pair +
    the planar gidx words give the routed G itself, hence the weight gradient."""
    B, H, Wv, xhat, Wt, G, amax = _problem(T, seed=9)
    Hp = H // 2
    dz = M.route(G, amax[..., :Wv])
    gp = M.cl_layout(G, Wv)
    words = M.g_idx_words(amax)
    assert words.shape == (B, Hp, 4, P) and words.dtype == np.uint32
    fields = (words[..., None] >> (2 * np.arange(16, dtype=np.uint32))) & 3
    assert np.array_equal(fields >> 1, np.broadcast_to(np.arange(16) & 1, fields.shape))      # element j lies in half j & 1 of its group
    assert (words[1, 0, 2, 5] >> (16 + 2 * 6)) & 3 == 2 * 0 + amax[1, 32 + 8 + 4 + 2, 0, 5]    # hf = 1, j = 6: channel 8 + 4 + 2
    r = M.routed_from_g_idx(gp, words)                                     # (B, Hp, 4, 352, 32), k = 2 channel + row
    want = np.stack([M.cl_layout(dz[:, :, par::2], Wv) for par in range(2)], -1).reshape(B, Hp, 4, P, 32)
    assert np.array_equal(r, want)
    wsp = M.pack_weights_sp(Wt)
    assert wsp.shape == (4, 3, 2, 13, 2, 64, 16) and wsp.size == M.W_SP_ELEMS
    # kh = 4 + r - 2 m - parity: zero for (m = 0, r = 1, parity 0): kh = 5, and for (m = 2, r = 0, parity 1): kh = -1
    assert not wsp[:, 0, 1, :, :, :, 0::2].any() and not wsp[:, 2, 0, :, :, :, 1::2].any()
    assert (wsp[:, 1] != 0).all() and (wsp != 0).sum() == 64 * 64 * 13 * (5 + 5)               # every row pair meets 5 kernel rows
    assert wsp[1, 1, 0, 2, 1, 32 + 3, 5] == 256 * Wt[16 + 10, 32 + 3, 4 - 2 - 1, 10]            # k = 21: co 16 + 10, parity 1
    rp = np.zeros((B, Hp + 2, 4, P + 12 * T, 32))
    rp[:, 1:1 + Hp, :, 6 * T:6 * T + P] = r
    dx = np.zeros((B, 64, H, Wv))
    for rr in range(2):
        for m in range(3):
            for kwf in range(13):
                wk = wsp[:, m, rr, kwf].reshape(4, 2, 2, 32, 16).transpose(0, 1, 3, 2, 4).reshape(4, 64, 32)   # [cb][ci][k]
                dx[:, :, rr::2] += np.einsum("bhcwk,cik->bihw", rp[:, m:m + Hp, :, kwf * T:kwf * T + Wv], wk)
    tol = 1e-12
    assert rel(dx / 256, M.conv64_dgrad(dz, Wt, T)) <= tol
    planar = M.gidx_words(amax)
    assert planar.shape == (B, 64, Hp, 22, 2) and planar.dtype == np.uint16
    dz_p = M.routed_from_gidx(gp, planar)
    assert np.array_equal(dz_p[..., :Wv], dz) and not dz_p[..., Wv:].any()
    assert rel(M.conv64_wgrad(dz_p[..., :Wv], xhat, T), M.conv64_wgrad(dz, xhat, T)) <= tol


# ==== the emulated arithmetic ======================================================================================================
def _conv_sel(B, H, Wv, pooled, n=48, seed=0):
    """Outputs (b, channel, row, w): the corners and edges of the image, and random ones."""
    g = np.random.default_rng(seed)
    rows = H // 2 if pooled else H
    b, c = g.integers(0, B, n), g.integers(0, 64, n)
    h, w = g.integers(0, rows, n), g.integers(0, Wv, n)
    h[:8], w[:8] = [0, 0, rows - 1, rows - 1, 0, rows - 1, 0, rows - 1], [0, Wv - 1, 0, Wv - 1, Wv // 2, Wv // 2, min(5, Wv - 1), max(Wv - 6, 0)]
    return b, c, h, w


def _w_sel(n=40, seed=0):
    g = np.random.default_rng(seed)
    co, ci, kh, kw = g.integers(0, 64, n), g.integers(0, 64, n), g.integers(0, 5, n), g.integers(0, 13, n)
    kh[:4], kw[:4] = [0, 4, 0, 4], [0, 12, 12, 0]
    return co, ci, kh, kw


def ratio(got, ref, bound):
    err = np.abs(np.asarray(got, f64) - np.asarray(ref, f64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / np.maximum(np.asarray(bound, f64), 1e-300))
    return float(np.max(r)) if r.size else 0.0


def _float_runs(B, H, Wv, T, order, defect=None, kinds=("fwd", "dgrad", "dgrad_sp", "wgrad", "wgrad_sp"), grads=None):
    """Every float comparison of the GPU file on the emulated kernels: yields (name, ratio to the per-element bound, error
    relative to the tensor's maximum)."""
    grads = grads or [("gauss", 0), ("gauss", 6), ("heavy", 0), ("heavy", 6)]
    if "fwd" in kinds:
        ops, ref = M.host_operands(B, H, Wv), M.float_fwd(B, H, Wv, T)
        sel = _conv_sel(B, H, Wv, True)
        got, _ = M.f16x3_emulate("fwd", dict(x_hi=ops["x_hi"], x_lo=ops["x_lo"], w_hi=ops["wf_hi"], w_lo=ops["wf_lo"],
                                             bias=M.float_inputs(B, H, Wv)["bias"]), B, H, Wv, T, sel, order, defect)
        b, c, hp, w = sel
        zb = np.maximum(ref["zbound"][b, c, 2 * hp, w], ref["zbound"][b, c, 2 * hp + 1, w])
        bound = zb + M.U * np.abs(M.float_inputs(B, H, Wv)["bias"].astype(f64))[c]
        yield "fwd", ratio(got, ref["out"][b, c, hp, w], bound), float(np.abs(got - ref["out"][b, c, hp, w]).max() / np.abs(ref["out"]).max())
    rps = 3
    for kind_g, shift in grads:
        ops = M.host_operands(B, H, Wv, kind_g, shift)
        for kind in kinds:
            if kind == "fwd":
                continue
            if kind.startswith("dgrad"):
                ref = M.float_dgrad(B, H, Wv, T, kind_g, shift)
                sel = _conv_sel(B, H, Wv, False)
                o = (dict(dz_hi=ops["dz_hi"], dz_lo=ops["dz_lo"], w_hi=ops["wflip_hi"], w_lo=ops["wflip_lo"]) if kind == "dgrad" else
                     dict(g_hi=ops["g_hi"], g_lo=ops["g_lo"], g_idx=ops["g_idx"], w_hi=ops["wsp_hi"], w_lo=ops["wsp_lo"]))
                got = M.f16x3_emulate(kind, dict(o, scale=ops["scale"]), B, H, Wv, T, sel, order, defect)
                want, bound, full = ref["dx"][sel], ref["bound"][sel], ref["dx"]
            else:
                ref = M.float_wgrad(B, H, Wv, T, kind_g, shift)
                sel = _w_sel()
                o = (dict(dz_hi=ops["dz_hi"], dz_lo=ops["dz_lo"]) if kind == "wgrad" else dict(g_hi=ops["g_hi"], g_lo=ops["g_lo"], gidx=ops["gidx"]))
                got = M.f16x3_emulate(kind, dict(o, x_hi=ops["x_hi"], x_lo=ops["x_lo"], scale=ops["scale"], rows_per_slab=rps),
                                      B, H, Wv, T, sel, order, defect)
                rows = rps if kind == "wgrad" else 2 * rps
                want, bound, full = ref["dW"][sel], M.wgrad_bound(ref, 3 * rows * Wv)[sel], ref["dW"]
            yield f"{kind}-{kind_g}-{shift}", ratio(got, want, bound), float(np.abs(got - want).max() / np.abs(full).max())


@pytest.mark.parametrize("order", ["natural", "sorted"])
@pytest.mark.parametrize("T", M.DILATIONS)
@pytest.mark.parametrize("B,H,Wv", M.ROUNDING_SHAPES)
def test_bounds_hold_for_the_arithmetic(B, H, Wv, T, order):
    """f16x3 arithmetic without a defect, in the natural order and with the largest terms first, stays within the per-element
    bounds the GPU tests gate the kernels with at tol = 1.0, and within the project's 1e-5 of the tensor's maximum."""
    tol = 1.0
    for name, r, relerr in _float_runs(B, H, Wv, T, order):
        assert r <= tol, (name, r)
        assert relerr < 1e-5, (name, relerr)


# ==== teeth ========================================================================================================================
_APPLIES = {"taps_not_mirrored": ("dgrad", "dgrad_sp"), "tie_to_odd_row": ("fwd",), "argmax_bit_inverted": ("dgrad_sp", "wgrad_sp"),
            "last_slab_skipped": ("wgrad", "wgrad_sp"), "scale_2s": ("dgrad", "dgrad_sp", "wgrad", "wgrad_sp")}
_ALL = ("fwd", "dgrad", "dgrad_sp", "wgrad", "wgrad_sp")
_INTEGER_ONLY = ("add_lo_lo", "tie_to_odd_row")       # 2^-22 of a term; ties do not happen on random floats


def _exact_runs(B, H, Wv, T, defect, kinds):
    """The exact comparisons of the GPU file on the emulated kernels: yields (name, number of selected outputs that differ)."""
    i, w, o = M.exact_inputs(B, H, Wv), M.exact_weights(), M.exact_grad_operands(B, H, Wv)
    bits = lambda a: np.ascontiguousarray(a, f32).view(np.int32)
    g = np.random.default_rng(1)
    if "fwd" in kinds:
        # all positions of four channels of the last clip (whose interior pooling pairs tie)
        b, c, hp, ww = (a.ravel() for a in np.meshgrid([B - 1], g.integers(0, 64, 4), np.arange(H // 2), np.arange(Wv), indexing="ij"))
        ref = M.exact_fwd(B, H, Wv, T)
        got, am = M.f16x3_emulate("fwd", dict(x_hi=i["x_hi"], x_lo=i["x_lo"], w_hi=w["fwd_hi"], w_lo=w["fwd_lo"], bias=i["bias"]),
                                  B, H, Wv, T, (b, c, hp, ww), "natural", defect)
        yield "fwd", int((bits(got) != bits(ref["out"][b, c, hp, ww])).sum() + (am != ref["amax"][b, c, hp, ww]).sum())
    sel = tuple(a.ravel() for a in np.meshgrid([0], [0, 41], np.arange(H), np.arange(Wv), indexing="ij"))
    for kind in ("dgrad", "dgrad_sp"):
        if kind in kinds:
            ops = (dict(dz_hi=o["dz_hi"], dz_lo=o["dz_lo"], w_hi=w["flip_hi"], w_lo=w["flip_lo"]) if kind == "dgrad" else
                   dict(g_hi=o["g_hi"], g_lo=o["g_lo"], g_idx=o["g_idx"], w_hi=w["sp_hi"], w_lo=w["sp_lo"]))
            got = M.f16x3_emulate(kind, dict(ops, scale=i["scale"]), B, H, Wv, T, sel, "natural", defect)
            yield kind, int((bits(got) != bits(M.exact_dgrad(B, H, Wv, T)["dx"][sel])).sum())
    wsel = tuple(a.ravel() for a in np.meshgrid([3, 40], [0, 9, 63], np.arange(5), np.arange(13), indexing="ij"))
    for kind in ("wgrad", "wgrad_sp"):
        if kind in kinds:
            ops = dict(dz_hi=o["dz_hi"], dz_lo=o["dz_lo"]) if kind == "wgrad" else dict(g_hi=o["g_hi"], g_lo=o["g_lo"], gidx=o["gidx"])
            got = M.f16x3_emulate(kind, dict(ops, x_hi=i["x_hi"], x_lo=i["x_lo"], scale=i["scale"], rows_per_slab=5 if kind == "wgrad" else 2),
                                  B, H, Wv, T, wsel, "natural", defect)
            yield kind, int((bits(got) != bits(M.exact_wgrad(B, H, Wv, T)["dW"][wsel])).sum())


def test_the_emulation_is_exact_on_the_integer_problems():
    """Without a defect the emulated kernels reproduce the fp64 references bit for bit (dilations 1 and 16)."""
    for T in (1, 16):
        for name, n_bad in _exact_runs(2, 6, 17, T, None, _ALL):
            assert n_bad == 0, (T, name, n_bad)


@pytest.mark.parametrize("defect", M.DEFECTS)
def test_defects_are_seen(defect):
    """Each deliberate deviation fails the comparison the GPU test makes, for every kernel it can occur in: the exact one on
    the integer problem, and (where it shows on random floats at all) the 1e-5 / per-element gates on the float problem."""
    B, H, Wv, T = 2, 6, 17, 2
    kinds = _APPLIES.get(defect, _ALL)
    seen = dict(_exact_runs(B, H, Wv, T, defect, kinds))
    assert set(seen) == set(kinds) and all(n > 0 for n in seen.values()), seen
    if defect in _INTEGER_ONLY:
        return
    # (the heavy-tailed gradients are powers of two, their lo halves zero: a kernel is held to the Gaussian problem as well)
    caught = {}
    for name, r, relerr in _float_runs(2, 4, 17, T, "natural", defect, kinds, grads=[("gauss", 0), ("heavy", 6)]):
        caught.setdefault(name.split("-")[0], []).append(r > 1.0 or relerr >= 1e-5)
    assert set(caught) == set(kinds) and all(any(v) for v in caught.values()), caught

"""CPU: the references of tests/helpers/general_refs64.py checked against torch.float64 ops on small random cases, at 1e-12
relative to each tensor's maximum -- the guard of the yardstick that kernel-level GPU tests of these entry points compare with.

* the helper imports numpy only
* F.conv2d(padding="same") with even and odd kernels and dilation, built from im2col2d + the strided GEMM; its autograd
  with respect to the input against col2im2d, with respect to the weight against the GEMM of the transposed layout
* nn.Conv1d with padding (k // 2) d, stride and dilation from tcn_im2col, its input gradient from tcn_col2im
* F.layer_norm, F.max_pool2d + F.prelu, F.batch_norm (training and eval), FiLM, the bin-mean head, nn.LSTM + its BPTT,
  the output layer with torch's broadcast -- forward and autograd
* the fp32 mode of the recurrences stays fp32 and lands within fp32 distance of the fp64 one
"""
import ast
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import general_refs64 as G

HELPER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "general_refs64.py")
T64 = torch.float64


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=T64, requires_grad=grad)


def _rel(got, want):
    want = np.asarray(want.detach().numpy() if isinstance(want, torch.Tensor) else want, np.float64)
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def test_helper_imports_only_numpy_and_math():
    tree = ast.parse(open(HELPER).read())
    roots = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            roots |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            assert node.level == 0, "relative import"
            roots.add(node.module.split(".")[0])
        elif isinstance(node, ast.Call) and getattr(node.func, "id", None) in ("__import__", "exec", "eval"):
            raise AssertionError("dynamic import / exec in the reference")
    assert roots <= {"numpy", "math"}, roots


def test_sgemm_addressing_groups_and_accumulate():
    g = np.random.default_rng(0)
    M, N, K, nb = 5, 7, 9, 5
    a, b = g.standard_normal((nb, K, M)), g.standard_normal((nb, N, K))          # both stored transposed
    c0 = g.standard_normal((3, N, M + 2))                                         # C transposed too, rows padded by 2
    out, written, mag, summed = G.sgemm(a, 0, 1, M, K * M, b, 0, 1, K, N * K, c0, 0, 1, M + 2, N * (M + 2), M, N, K, nb, 2, 1)
    want = c0.copy()
    for grp, ids in enumerate(([0, 1], [2, 3], [4])):
        want[grp, :, :M] += sum(a[i].T @ b[i].T for i in ids).T
    assert _rel(out.reshape(want.shape), want) <= 1e-12
    w = written.reshape(want.shape)
    assert w[:, :, :M].all() and not w[:, :, M:].any()
    assert sorted(set(summed[written])) == [1, 2] and (mag[written] > 0).all()
    # broadcast A (a_bs = 0), offset base pointers, no accumulate
    out, written, _, _ = G.sgemm(a, 3, M, 1, 0, b, K, K, 1, N * K, np.full(2 * M * N, np.nan), 0, N, 1, M * N, M, 4, 2, 2, 1, 0)
    A = np.stack([a.ravel()[3 + m * M:3 + m * M + 2] for m in range(M)])
    for i in range(2):
        Bm = np.stack([[b.ravel()[K + i * N * K + k * K + n] for n in range(4)] for k in range(2)])
        assert _rel(out.reshape(2, M, N)[i, :, :4], A @ Bm) <= 1e-12
    assert np.isnan(out[~written]).all() and written.sum() == 2 * M * 4


@pytest.mark.parametrize("kh,kw,dh,dw", [(1, 1, 1, 1), (3, 3, 1, 1), (2, 4, 1, 1), (2, 4, 2, 3), (5, 13, 1, 2), (4, 1, 2, 1)])
def test_conv2d_same_from_im2col_and_its_autograd(kh, kw, dh, dw):
    g = np.random.default_rng(kh * 100 + kw * 10 + dh)
    nb, Cin, Cout, H, W = 2, 3, 4, 5, 9
    x, w = g.standard_normal((nb, Cin, H, W)), g.standard_normal((Cout, Cin, kh, kw))
    gy = g.standard_normal((nb, Cout, H, W))
    xt, wt = _t(x, True), _t(w, True)
    y = F.conv2d(xt, wt, padding="same", dilation=(dh, dw))
    y.backward(_t(gy))
    pt, pl = G.same_pad(kh, dh), G.same_pad(kw, dw)
    Kk, HW = Cin * kh * kw, H * W
    col = G.im2col2d(x, kh, kw, dh, dw, pt, pl)
    # the product's forward call: z[b] (Cout, HW) = W (Cout, K) col[:, b HW:(b + 1) HW]
    z, written, _, _ = G.sgemm(w, 0, Kk, 1, 0, col, 0, nb * HW, 1, HW, np.zeros(nb * Cout * HW), 0, HW, 1, Cout * HW, Cout, HW, Kk, nb, 1, 0)
    assert written.all() and _rel(z.reshape(nb, Cout, H, W), y) <= 1e-12
    # weight gradient: dW (Cout, K) = sum over clips of dz[b] (Cout, HW) col_b^T, reduced inside one group
    dw_, _, _, _ = G.sgemm(gy, 0, HW, 1, Cout * HW, col, 0, 1, nb * HW, HW, np.zeros(Cout * Kk), 0, Kk, 1, 0, Cout, Kk, HW, nb, nb, 0)
    assert _rel(dw_.reshape(w.shape), wt.grad) <= 1e-12
    # data gradient: dcol (K, nb HW) = W^T dz, then the transposed gather
    dcol, _, _, _ = G.sgemm(w, 0, 1, Kk, 0, gy, 0, HW, 1, Cout * HW, np.zeros(Kk * nb * HW), 0, nb * HW, 1, HW, Kk, HW, Cout, nb, 1, 0)
    dx = G.col2im2d(dcol.reshape(Kk, nb * HW), nb, Cin, H, W, kh, kw, dh, dw, pt, pl)
    assert _rel(dx, xt.grad) <= 1e-12
    # the adjoint identity of the two gathers, with an explicit (causal) padding
    pt2 = dh * (kh - 1)
    d = g.standard_normal((Kk, nb * HW))
    lhs = float((G.col2im2d(d, nb, Cin, H, W, kh, kw, dh, dw, pt2, 0) * x).sum())
    rhs = float((d * G.im2col2d(x, kh, kw, dh, dw, pt2, 0)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(rhs), 1.0)


@pytest.mark.parametrize("ksz,dil,stride,T", [(1, 1, 1, 5), (3, 1, 2, 11), (4, 4, 3, 20), (9, 4, 1, 6), (3, 1, 1, 1), (4, 1, 2, 17)])
def test_conv1d_from_tcn_im2col_and_its_autograd(ksz, dil, stride, T):
    g = np.random.default_rng(ksz * 31 + dil * 7 + stride)
    B, C, Co = 2, 3, 4
    x = np.zeros((B, C, G.PITCH))
    x[:, :, :T] = g.standard_normal((B, C, T))
    w = g.standard_normal((Co, C, ksz))
    xt = _t(x[:, :, :T], True)
    y = F.conv1d(xt, _t(w), stride=stride, dilation=dil, padding=(ksz // 2) * dil)
    To = G.conv1d_out_len(T, ksz, dil, stride)
    assert y.shape[-1] == To
    col = G.tcn_im2col(x, None, T, To, ksz, dil, stride)
    z = np.einsum("ok,kbt->bot", w.reshape(Co, C * ksz), col.reshape(C * ksz, B, To))
    assert _rel(z, y) <= 1e-12
    gy = g.standard_normal((B, Co, To))
    y.backward(_t(gy))
    dcol = np.einsum("ok,bot->kbt", w.reshape(Co, C * ksz), gy).reshape(C * ksz, B * To)
    assert _rel(G.tcn_col2im(dcol, B, C, T, To, ksz, dil, stride), xt.grad) <= 1e-12
    # with statistics: the normalisation comes before the zero padding
    st = np.stack([x[:, :, :T].mean((1, 2)), 1.0 / np.sqrt(x[:, :, :T].var((1, 2)) + 1e-5)], -1)
    xn = F.layer_norm(_t(x[:, :, :T]), (C, T), eps=1e-5)
    yn = F.conv1d(xn, _t(w), stride=stride, dilation=dil, padding=(ksz // 2) * dil)
    coln = G.tcn_im2col(x, st, T, To, ksz, dil, stride)
    zn = np.einsum("ok,kbt->bot", w.reshape(Co, C * ksz), coln.reshape(C * ksz, B, To))
    assert float(np.abs(zn - yn.numpy()).max()) <= 1e-12 * max(float(yn.abs().max()), 1.0)


def test_layer_norm_rows_and_tcn_planes():
    g = np.random.default_rng(3)
    x, gy = g.standard_normal((3, 37)) * 3 + 1, g.standard_normal((3, 37))
    xt = _t(x, True)
    y = F.layer_norm(xt, (37,), eps=1e-5)
    y.backward(_t(gy))
    yr, st = G.rowln_fwd(x, 1e-5)
    assert _rel(yr, y) <= 1e-12
    assert _rel(st[:, 0], x.mean(-1)) <= 1e-12 and _rel(st[:, 1], 1 / np.sqrt(x.var(-1) + 1e-5)) <= 1e-12
    dx, _ = G.rowln_bwd(gy, yr, st)
    assert _rel(dx, xt.grad) <= 1e-12
    assert _rel(G.row_sums(x)[0], x.sum(-1)) <= 1e-12
    # LayerNorm([C, T]) of a (B, C, 352) plane with an extra gradient around it
    B, C, T = 2, 3, 11
    xp, gp, add = (np.zeros((B, C, G.PITCH)) for _ in range(3))
    xp[:, :, :T], gp[:, :, :T], add[:, :, :T] = (g.standard_normal((B, C, T)) for _ in range(3))
    xt = _t(xp[:, :, :T], True)
    (F.layer_norm(xt, (C, T), eps=1e-5) * _t(gp[:, :, :T])).sum().backward()
    stp = np.stack([xp[:, :, :T].mean((1, 2)), 1 / np.sqrt(xp[:, :, :T].var((1, 2)) + 1e-5)], -1)
    dxp, _, _ = G.tcn_ln_bwd(xp, gp, stp, add, T)
    assert _rel(dxp[:, :, :T], xt.grad + _t(add[:, :, :T])) <= 1e-12 and not dxp[:, :, T:].any()


@pytest.mark.parametrize("use_slope,use_res", [(True, True), (True, False), (False, True)])
def test_tcn_act_and_prelu_res(use_slope, use_res):
    g = np.random.default_rng(4)
    B, C, T = 2, 3, 13
    z, res, gy = (np.zeros((B, C, G.PITCH)) for _ in range(3))
    z[:, :, :T], res[:, :, :T], gy[:, :, :T] = (g.standard_normal((B, C, T)) for _ in range(3))
    bias, slope = g.standard_normal(C), g.uniform(0.05, 0.5, C)
    zt, bt, st = _t(z[:, :, :T], True), _t(bias, True), _t(slope, True)
    zb_t = zt + bt[None, :, None]
    y_t = F.prelu(zb_t, st) if use_slope else zb_t
    if use_res:
        y_t = y_t + _t(res[:, :, :T])
    y_t.backward(_t(gy[:, :, :T]))
    zb, y = G.tcn_act_fwd(z, bias, slope if use_slope else None, res if use_res else None, T)
    assert _rel(y[:, :, :T], y_t) <= 1e-12 and not y[:, :, T:].any()
    dz, part, mag = G.tcn_act_bwd(gy, zb, slope if use_slope else None, T)
    assert _rel(dz[:, :, :T], zt.grad) <= 1e-12 and not dz[:, :, T:].any()
    assert _rel(part[:, 0].reshape(B, C).sum(0), bt.grad) <= 1e-12
    if use_slope:
        assert _rel(part[:, 1].reshape(B, C).sum(0), st.grad) <= 1e-12
    else:
        assert not part[:, 1].any()
    assert (mag >= np.abs(part) - 1e-15).all()
    # the dense general-TCN variant
    a = z[:, :, :T]
    at = _t(a, True)
    yt = (F.prelu(at, st) if use_slope else at) + (_t(res[:, :, :T]) if use_res else 0)
    assert _rel(G.prelu_res_fwd(a, slope if use_slope else None, res[:, :, :T] if use_res else None), yt) <= 1e-12
    if use_slope:
        st.grad = None
        yt.backward(_t(gy[:, :, :T]))
        da, p, _ = G.prelu_res_bwd(gy[:, :, :T], a, slope)
        assert _rel(da, at.grad) <= 1e-12 and _rel(p.reshape(B, C).sum(0), st.grad) <= 1e-12


def test_prelu_conventions_at_zero():
    v = np.array([0.0, -0.0, 1.0, -1.0])
    assert np.array_equal(G.prelu(v, 0.25), [0.0, -0.0, 1.0, -0.25])
    da, part, _ = G.prelu_res_bwd(np.ones((1, 1, 4)), v.reshape(1, 1, 4), [0.25])
    assert G.prelu_res_bwd(np.ones((1, 1, 4)), v.reshape(1, 1, 4), [0.25], dtype=np.float32)[0].dtype == np.float32
    assert G.film_bwd(np.ones((1, 1, 4)), v.reshape(1, 1, 4), np.ones((1, 2)), dtype=np.float32)[0].dtype == np.float32
    assert np.array_equal(da.ravel(), [0.25, 0.25, 1.0, 0.25]) and part[0] == -1.0           # torch: a > 0 ? 1 : slope


@pytest.mark.parametrize("p,H", [(1, 3), (2, 7), (3, 7), (3, 8), (2, 8)])
def test_pool_prelu_against_max_pool2d_and_prelu(p, H):
    g = np.random.default_rng(p * 10 + H)
    B, C, W = 2, 3, 6
    z = np.round(g.standard_normal((B * C, H, W)) * 4) / 4                        # coarse values: exact ties inside windows
    bias, slope, gy = g.standard_normal(C), g.uniform(0.05, 0.5, C), g.standard_normal((B * C, H // p, W))
    zt, bt, st = _t(z.reshape(B, C, H, W), True), _t(bias, True), _t(slope, True)
    v_t, idx = F.max_pool2d(zt + bt[None, :, None, None], (p, 1), return_indices=True)
    out_t = F.prelu(v_t, st)
    out_t.backward(_t(gy.reshape(B, C, H // p, W)))
    v, out, amax = G.pool_prelu_fwd(z, bias, C, p, slope)
    assert _rel(v, v_t.reshape(v.shape)) <= 1e-12 and _rel(out, out_t.reshape(out.shape)) <= 1e-12
    rows = (idx.numpy().reshape(B * C, H // p, W) // W) - np.arange(H // p)[None, :, None] * p
    assert np.array_equal(amax, rows)                                             # aten keeps the first maximum
    dz, part, _ = G.pool_prelu_bwd(gy, v, amax, C, H, p, slope)
    assert _rel(dz, zt.grad.reshape(dz.shape)) <= 1e-12
    assert not dz[:, (H // p) * p:].any()
    assert _rel(part[:, 0].reshape(B, C).sum(0), bt.grad) <= 1e-12 and _rel(part[:, 1].reshape(B, C).sum(0), st.grad) <= 1e-12


@pytest.mark.parametrize("mode", ["both", "out", "latent"])
def test_binmean_head(mode):
    g = np.random.default_rng(6)
    B, C, H, W, L = 2, 5, 4, 7, 3
    x, wout, bout = g.standard_normal((B, C, H, W)), g.standard_normal((L, C)), g.standard_normal(L)
    d_out, d_lat = g.standard_normal((B, L, W)), g.standard_normal((B, C, W))
    xt = _t(x, True)
    lat_t = xt.mean(2)
    out_t = torch.sigmoid(F.conv1d(lat_t, _t(wout)[:, :, None], _t(bout)))
    latent, out, _ = G.binmean_head_fwd(x, wout, bout)
    assert _rel(latent, lat_t) <= 1e-12 and _rel(out, out_t) <= 1e-12
    loss = 0
    if mode != "latent":
        loss = loss + (out_t * _t(d_out)).sum()
    if mode != "out":
        loss = loss + (lat_t * _t(d_lat)).sum()
    loss.backward()
    ds, dx, mag = G.binmean_head_bwd(d_out if mode != "latent" else None, d_lat if mode != "out" else None, out, wout, B, C, H, W)
    assert _rel(dx, xt.grad) <= 1e-12 and (mag + 1e-15 >= np.abs(dx[:, :, 0]) * H).all()
    if mode == "latent":
        assert not ds.any()
    else:
        assert _rel(ds, _t(d_out) * out_t * (1 - out_t)) <= 1e-12


@pytest.mark.parametrize("train", [True, False])
def test_batch_norm_and_film(train):
    g = np.random.default_rng(7)
    B, C, T = 3, 4, 9
    z, gy, gb = g.standard_normal((B, C, T)) * 2 + 1, g.standard_normal((B, C, T)), g.standard_normal((B, 2 * C))
    zt, gbt = _t(z, True), _t(gb, True)
    if train:
        xh_t = F.batch_norm(zt, None, None, training=True, eps=1e-5)
        stats, _ = G.chan_stats(z)
        assert _rel(stats[:, 0], z.mean((0, 2))) <= 1e-12 and _rel(stats[:, 1], z.var((0, 2))) <= 1e-12
    else:
        rm, rv = g.standard_normal(C), g.uniform(0.5, 2, C)
        xh_t = F.batch_norm(zt, _t(rm), _t(rv), training=False, eps=1e-5)
        stats = np.stack([rm, rv], -1)
    norm = np.stack([stats[:, 0], 1 / np.sqrt(stats[:, 1] + 1e-5)], -1)
    a_t = xh_t * gbt[:, :C, None] + gbt[:, C:, None]
    a_t.backward(_t(gy))
    xhat = G.chan_norm_fwd(z, norm)
    assert _rel(xhat, xh_t) <= 1e-12 and _rel(G.film_fwd(xhat, gb), a_t) <= 1e-12
    dxh, dgb, mag = G.film_bwd(gy, xhat, gb)
    assert _rel(dgb, gbt.grad) <= 1e-12 and (mag >= np.abs(dgb) - 1e-15).all()
    dz, _ = G.chan_norm_bwd(dxh, xhat, norm, train)
    assert _rel(dz, zt.grad) <= 1e-12


@pytest.mark.parametrize("Hn,T", [(1, 3), (7, 5), (12, 1)])
def test_lstm_recurrence_and_bptt_against_nn_lstm(Hn, T):
    g = np.random.default_rng(Hn)
    B, D = 2, 3
    lstm = torch.nn.LSTM(D, Hn, batch_first=True).double()
    u = g.standard_normal((B, T, D))
    h0, c0 = g.standard_normal((B, Hn)) * 0.5, g.standard_normal((B, Hn)) * 0.5
    dhfc = g.standard_normal((B, T, Hn))
    w_ih, w_hh, b_ih, b_hh = (p.detach().numpy() for p in (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0))
    ut = _t(u, True)
    hs, (h1, c1) = lstm(ut, (_t(h0)[None], _t(c0)[None]))
    (hs * _t(dhfc)).sum().backward()
    zin = u @ w_ih.T
    stash, h1r, c1r = G.lstmg_fwd(zin, b_ih, b_hh, w_hh, h0, c0)
    assert _rel(stash[:, :, 5], hs) <= 1e-12 and _rel(h1r, h1[0]) <= 1e-12 and _rel(c1r, c1[0]) <= 1e-12
    dgate = G.lstmg_bwd(stash, dhfc, w_hh, c0)
    # every parameter gradient is a product of dgate: the bias, the input weights and the recurrent weights pin all of it
    assert _rel(dgate.sum((0, 1)), lstm.bias_ih_l0.grad) <= 1e-12
    assert _rel(np.einsum("btg,btd->gd", dgate, u), lstm.weight_ih_l0.grad) <= 1e-12
    hprev = np.concatenate([h0[:, None], stash[:, :-1, 5]], 1)
    assert _rel(np.einsum("btg,bth->gh", dgate, hprev), lstm.weight_hh_l0.grad) <= 1e-12
    assert _rel(dgate @ w_ih, ut.grad) <= 1e-12
    # the fp32 yardstick: same formulae, fp32 throughout, within fp32 distance of the fp64 run
    s32, h32, _ = G.lstmg_fwd(zin.astype(np.float32), b_ih, b_hh, w_hh, h0, c0, dtype=np.float32)
    d32 = G.lstmg_bwd(stash.astype(np.float32), dhfc, w_hh, c0, dtype=np.float32)
    assert s32.dtype == np.float32 and h32.dtype == np.float32 and d32.dtype == np.float32
    assert 0 < float(np.abs(s32 - stash).max()) <= 1e-5 and float(np.abs(d32 - dgate).max()) <= 1e-5
    # ... and truly fp32 inside: step 0 equals an explicit fp32 step bit for bit (an fp64 intermediate would round differently
    # somewhere among these values), and the activations keep their argument's precision
    f = np.float32
    one, c32 = f(1), c0.astype(f)
    pre = zin.astype(f)[:, 0] + b_ih.astype(f) + b_hh.astype(f) + h0.astype(f) @ w_hh.astype(f).T
    assert pre.dtype == f and G.sigmoid(pre).dtype == f and G.sigmoid(pre.astype(np.float64)).dtype == np.float64
    gi, gf, go = (one / (one + np.exp(-pre[:, q * Hn:(q + 1) * Hn])) for q in (0, 1, 3))
    gg = np.tanh(pre[:, 2 * Hn:3 * Hn])
    cn = gf * c32 + gi * gg
    hn = go * np.tanh(cn)
    for q, val in enumerate((gi, gf, gg, go, cn, hn)):
        assert val.dtype == f and np.array_equal(val.view(np.int32), s32[:, 0, q].view(np.int32)), q


@pytest.mark.parametrize("in_ch,out_ch", [(1, 1), (2, 2), (1, 3), (3, 1)])
def test_lstm_output_layer_broadcast(in_ch, out_ch):
    g = np.random.default_rng(in_ch * 4 + out_ch)
    B, T = 2, 6
    fc, bias, x = g.standard_normal((B, T, out_ch)), g.standard_normal(out_ch), g.standard_normal((B, in_ch, T))
    Co = max(in_ch, out_ch)
    dy = g.standard_normal((B, Co, T))
    fct = _t(fc, True)
    y_t = torch.tanh((fct + _t(bias)).transpose(1, 2) + _t(x))
    y_t.backward(_t(dy))
    y = G.lstmg_out_fwd(fc, bias, x)
    assert y.shape == (B, Co, T) and _rel(y, y_t) <= 1e-12
    assert _rel(G.lstmg_out_bwd(dy, y, out_ch), fct.grad) <= 1e-12
    assert G.lstmg_out_fwd(fc, bias, x, dtype=np.float32).dtype == np.float32

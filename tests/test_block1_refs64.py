"""CPU: the fp64 references of tests/helpers/block1_refs64.py against torch's fp64 conv2d / layer_norm / prelu / max_pool2d
autograd, to 1e-12 of the tensor's maximum, and the two operand layouts against the convolution they must reproduce -- so that
a wrong reference cannot certify a wrong kernel (tests/test_gpu_block1_units.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import block1_refs64 as R

f64 = np.float64


def rel(got, ref):
    ref = np.asarray(ref, f64)
    return float(np.abs(np.asarray(got, f64) - ref).max() / max(float(np.abs(ref).max()), 1e-300))


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, f64))


@pytest.mark.parametrize("B,H,W", [(1, 2, 1), (2, 6, 17), (3, 4, 30)])
def test_block1_forward_and_weight_gradient(B, H, W):
    g = np.random.default_rng(B * 100 + H * 10 + W)
    x = g.standard_normal((B, 2, H, W)) * 2.0 + 0.5
    Wt, bias, Gc = g.standard_normal((64, 2, 5, 13)) / np.sqrt(130), g.standard_normal(64) * 0.1, g.standard_normal((B, 64, H // 2, W))
    stats = R.plane_stats(x)
    xhat = R.normalise(x, stats)
    out, amax, z = R.conv1_pool_fwd(xhat, Wt, bias)
    w_t = t64(Wt).requires_grad_(True)
    xhat_t = F.layer_norm(t64(x), (H, W), eps=1e-5)
    z_t = F.conv2d(xhat_t, w_t, t64(bias), padding="same")
    p_t, idx = F.max_pool2d(z_t, (2, 1), return_indices=True)
    (p_t * t64(Gc)).sum().backward()
    tol = 1e-12
    assert rel(xhat, xhat_t.numpy()) <= tol
    assert rel(z + bias[None, :, None, None], z_t.detach().numpy()) <= tol
    assert rel(out, p_t.detach().numpy()) <= tol
    rows = (idx.numpy() // W) % 2                                          # flat index into the (H, W) plane -> row parity
    gap = np.abs(z[:, :, 1::2] - z[:, :, 0::2])
    assert np.array_equal(amax[gap > 1e-9], rows[gap > 1e-9].astype(np.uint8))
    assert rel(R.conv1_wgrad(R.route(Gc, amax), xhat), w_t.grad.numpy()) <= tol


def test_pool_tie_rule_and_route():
    z = np.zeros((1, 1, 4, 3))
    z[0, 0, :, 0] = [1, 1, 2, 3]
    z[0, 0, :, 1] = [5, 4, -0.0, 0.0]
    z[0, 0, :, 2] = [4, 5, 7, 7]
    pooled, amax = R.pool21(z)
    assert amax.tolist() == [[[[0, 0, 1], [1, 0, 0]]]] and pooled.tolist() == [[[[1, 5, 5], [3, 0, 7]]]]
    dz = R.route(np.full((1, 1, 2, 3), 9.0), amax)
    assert dz[0, 0].tolist() == [[9, 9, 0], [0, 0, 9], [0, 9, 9], [9, 0, 0]]


def test_kvec_layouts_reproduce_the_convolution():
    """sum over (kw, k) of wk[kw][k] xk[b][h][w + kw - 6][k] / 256 == the convolution; zeros exactly where the ABI says."""
    g = np.random.default_rng(5)
    B, H, Wv = 2, 6, 9
    xhat, Wt = g.standard_normal((B, 2, H, Wv)), g.standard_normal((64, 2, 5, 13))
    wide = np.full((B, 2, H, Wv + 3), 1e30)                                # columns beyond Wv must not show
    wide[..., :Wv] = xhat
    xk, wk = R.kvec_layout(wide, Wv), R.kvec_weights(Wt)
    assert xk.shape == (B, H, R.PITCH, 16) and wk.shape == (13, 2, 64, 8)
    assert not xk[:, :, Wv:].any() and not xk[..., 10:].any() and not wk[:, 1, :, 2:].any()
    assert not xk[:, 0, :, :4].any() and not xk[:, 1, :, :2].any() and not xk[:, H - 1, :, 6:].any() and not xk[:, H - 2, :, 8:].any()
    assert xk[1, 2, 3, 2 * 3 + 1] == xhat[1, 1, 3, 3] and wk[4, 1, 7, 1] == 256 * Wt[7, 1, 4, 4]
    wk16 = wk.transpose(0, 1, 3, 2).reshape(13, 16, 64)                     # [kw][k][co]
    xp = np.zeros((B, H, R.PITCH + 12, 16))
    xp[:, :, 6:6 + R.PITCH] = xk
    z = sum(np.einsum("bhwk,kc->bchw", xp[:, :, kw:kw + Wv], wk16[kw]) for kw in range(13)) / 256
    tol = 1e-12
    assert rel(z, R.conv1(xhat, Wt)) <= tol


def test_split16_pairs():
    g = np.random.default_rng(6)
    v = (g.standard_normal(4096) * 2.0 ** g.integers(-12, 10, 4096)).astype(np.float32)
    hi, lo = R.split16(v)
    assert hi.dtype == np.float16 and lo.dtype == np.float16
    err = np.abs(hi.astype(f64) + lo.astype(f64) - v.astype(f64))
    assert (err <= 2.0 ** -22 * np.abs(v) + 2.0 ** -25).all()
    h2, l2 = R.unpack_pair(R.pack_pair(hi, lo))
    assert np.array_equal(h2.view(np.uint16), hi.view(np.uint16)) and np.array_equal(l2.view(np.uint16), lo.view(np.uint16))
    assert R.pack_pair(np.float16(1.0), np.float16(-2.0)) == 0xC0003C00


@pytest.mark.parametrize("B,C,H,W", [(1, 1, 1, 2), (2, 5, 4, 17)])
def test_ln_prelu_bwd(B, C, H, W):
    g = np.random.default_rng(B + C + H + W)
    p, D, slope = g.standard_normal((B, C, H, W)), g.standard_normal((B, C, H, W)), g.uniform(0.05, 0.5, C)
    p[0, 0, 0, 0] = 0.0                                                    # the kink: the slope branch
    stats = R.plane_stats(R.prelu(p, slope[None, :, None, None]))
    r = R.ln_prelu_bwd(p, D, stats, slope)
    p_t, s_t = t64(p).requires_grad_(True), t64(slope).requires_grad_(True)
    xhat_t = F.layer_norm(F.prelu(p_t, s_t), (H, W), eps=1e-5)
    (xhat_t * t64(D)).sum().backward()
    tol = 1e-12
    assert rel(r["xhat"], xhat_t.detach().numpy()) <= tol
    assert rel(r["G"], p_t.grad.numpy()) <= tol
    assert rel(r["dslope"].sum(0), s_t.grad.numpy()) <= tol
    # the plane sum of G cancels (exactly, where no element takes the slope branch): relative to the sum of the magnitudes
    assert float(np.abs(r["gsum"] - p_t.grad.numpy().sum((2, 3))).max() / r["gsum_mag"].max()) <= tol
    again = R.ln_prelu_bwd(p, D, stats, slope, m12=(r["m1"], r["m2"]))
    assert np.array_equal(again["G"], r["G"])
    assert (np.abs(r["G"]) <= r["G_mag"] * (1 + 1e-12)).all()


@pytest.mark.parametrize("B,C,Hl,W,L,with_dl", [(1, 3, 1, 1, 1, True), (2, 5, 4, 9, 4, False), (3, 64, 8, 5, 2, True)])
def test_head_fwd_bwd(B, C, Hl, W, L, with_dl):
    g = np.random.default_rng(B + C + Hl + W + L)
    p6, slope = g.standard_normal((B, C, Hl, W)), g.uniform(0.05, 0.5, C)
    p6[0, 0, 0, 0] = 0.0
    wout, bout = g.standard_normal((L, C)) / np.sqrt(C), g.standard_normal(L) * 0.1
    d_out, d_lat = g.standard_normal((B, L, W)), g.standard_normal((B, C, W))
    f = R.head_fwd(p6, slope, wout, bout)
    r = R.head_bwd(p6, slope, wout, f["latent"], f["out"], d_out, d_lat if with_dl else None)
    p_t, s_t, w_t, b_t = (t64(a).requires_grad_(True) for a in (p6, slope, wout, bout))
    lat_t = F.prelu(p_t, s_t).mean(2)
    out_t = torch.sigmoid(F.conv1d(lat_t, w_t[:, :, None], b_t))
    loss = (out_t * t64(d_out)).sum()
    if with_dl:
        loss = loss + (lat_t * t64(d_lat)).sum()
    loss.backward()
    tol = 1e-12
    assert rel(f["latent"], lat_t.detach().numpy()) <= tol
    assert rel(f["out"], out_t.detach().numpy()) <= tol
    assert rel(r["G6"], p_t.grad.numpy()) <= tol
    assert rel(r["dwout"].sum(0), w_t.grad.numpy()) <= tol
    assert rel(r["dbout"].sum(0), b_t.grad.numpy()) <= tol
    assert rel(r["dslope"].sum(0), s_t.grad.numpy()) <= tol


def test_stats_rows():
    g = np.random.default_rng(8)
    out, bias, slope = g.standard_normal((2, 64, 3, 7)), g.standard_normal(64), g.uniform(0.05, 0.5, 64)
    s, m = R.stats_rows(out, bias, slope)
    assert s.shape == (2, 3, 64, 2) and m.shape == (2, 3, 64, 2)
    y = F.prelu(t64(out), t64(slope)).numpy() - F.prelu(t64(bias)[None, :, None, None], t64(slope)).numpy()
    tol = 1e-12
    assert rel(s[1, 2, 5], [y[1, 5, 2].sum(), (y[1, 5, 2] ** 2).sum()]) <= tol
    assert rel(s[..., 0], y.sum(-1).transpose(0, 2, 1)) <= tol and (np.abs(s) <= m * (1 + 1e-12)).all()

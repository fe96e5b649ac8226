"""The forward convolution of blocks 5 and 6 (dilation 8 and 16), `mx_conv_block_fwd_f16`, against an fp64 CPU evaluation of
LayerNorm'd input -> conv 5x13 (dilation (1, T), same padding) -> bias -> max-pool (2, 1).

At these dilations the entry point runs the LDS-DMA kernel on a ring of three patch-row slots, which leaves out the matrix
instructions whose patch tile lies entirely in the zero halo.  The shapes are the smallest at which that kernel can go wrong:

  a  1 x  2 x  17   one row pair, every halo row outside the image, every column tile touches the halo
  b  2 x  4 x 351   both workgroups of a clip are edge workgroups; the widest frame count the sparse routes take
  c  2 x  8 x 345   the shipped frame count; interior and edge row pairs
  d  3 x 16 x  88   the rows of a workgroup pass through every ring slot; odd batch
  e  2 x  6 x 345   operand zero except the outermost 100 columns on each side: all that reaches the outer column tiles comes
                    through the taps next to the halo ones, so a tile left out wrongly shows here.  This case also has to match
                    the exact-fp32 kernel (`mx_conv_block_fwd`, the route MODEX_CONV_PRECISION=f32 selects) on the same input.

Gates are those of tests/test_gpu_conv_units.py::test_block_f16x3_kernels for this entry point: values to 1e-5 of the tensor's
maximum, argmax bytes equal to the reference's but for near-ties (fewer than 1e-4 of them), the LayerNorm statistics from
`stats_part` to 2e-6, and identical outputs with `slope_out` / `stats_part` given and NULL."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
PITCH = 352

CASES = {
    "a": (1, 2, 17),
    "b": (2, 4, 351),
    "c": (2, 8, 345),
    "d": (3, 16, 88),
    "e": (2, 6, 345),
}


def to_planes(x, dev):
    """(B,C,H,W) cpu -> (B,C,H,352) device, zero padded."""
    out = torch.zeros(x.shape[:-1] + (PITCH,), dtype=x.dtype)
    out[..., :x.size(-1)] = x
    return out.to(dev).contiguous()


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def ref64(x_in, slope_prev, w, b, T, identity_ln):
    """fp64 reference: (pooled pre-activation, the two rows of every pooling pair)."""
    x = x_in.double()
    if not identity_ln:
        x = F.prelu(x, slope_prev.double())
        x = F.layer_norm(x, x.shape[-2:], eps=1e-5)
    z = F.conv2d(x, w.double(), b.double(), dilation=(1, T), padding="same")
    return F.max_pool2d(z, (2, 1)), z


@pytest.mark.parametrize("T", [8, 16])
@pytest.mark.parametrize("case", sorted(CASES))
def test_fwd_dilated(dev, case, T):
    from mod_extraction_amd import _hip, models as am
    B, H, W = CASES[case]
    torch.manual_seed(1000 * T + 10 * H + W + B)
    identity_ln = case == "e"
    w = torch.randn(64, 64, 5, 13) / np.sqrt(64 * 65)
    b = torch.randn(64) * 0.1
    st = _hip.stream()
    if identity_ln:
        # the operand itself is chosen: mean 0, rstd 1 and slope 1 make the preparation the identity
        x_in = torch.randn(B, 64, H, W) * 0.7 + 0.1
        x_in[..., 100:W - 100] = 0.0
        slope_prev = torch.ones(64)
        stats = torch.tensor([0.0, 1.0]).repeat(B, 64, 1).to(dev).contiguous()
    else:
        x_in = torch.randn(B, 64, H, W) * 0.7 + 0.1
        slope_prev = torch.rand(64) * 0.4 + 0.05
        stats = torch.empty((B, 64, 2), device=dev)
    x_d, sl_d, b_d = to_planes(x_in, dev), slope_prev.to(dev), b.to(dev)
    if not identity_ln:
        _hip.call("mx_plane_stats", _hip.ptr(x_d), _hip.ptr(sl_d), B, 64, H, W, 1e-5, _hip.ptr(stats), st)
    p_r, z_r = ref64(x_in, slope_prev, w, b, T, identity_ln)

    x_hi = torch.empty((B, H, 4, PITCH, 16), device=dev, dtype=torch.float16)
    x_lo = torch.empty_like(x_hi)
    _hip.call("mx_conv_prep_fwd_f16", _hip.ptr(x_d), _hip.ptr(stats), _hip.ptr(sl_d), B, H, W, _hip.ptr(x_hi), _hip.ptr(x_lo), st)
    w_hi, w_lo = am._pack_f16(w.to(dev), 0)
    Hp = H // 2
    p = torch.full((B, 64, Hp, PITCH), float("nan"), device=dev)
    amax = torch.full((B, 64, Hp, PITCH), 255, device=dev, dtype=torch.uint8)
    sl_out = (torch.rand(64) * 0.4 + 0.05).to(dev)
    st_part = torch.full((B, Hp, 64, 2), float("nan"), device=dev)
    _hip.call("mx_conv_block_fwd_f16", _hip.ptr(x_hi), _hip.ptr(x_lo), _hip.ptr(w_hi), _hip.ptr(w_lo), _hip.ptr(b_d),
              B, H, W, T, _hip.ptr(p), _hip.ptr(amax), _hip.ptr(sl_out), _hip.ptr(st_part), st)
    # ---- values
    err = rel(p.cpu()[..., :W].double(), p_r)
    print(f"case {case} T {T}: value error {err:.3g} of the maximum")
    assert err < 1e-5
    assert bool((p[..., W:] == 0).all())
    # ---- argmax bytes: the reference's, near-ties aside
    am_r = (z_r[:, :, 1::2] > z_r[:, :, 0::2]).to(torch.uint8)
    mism = amax.cpu()[..., :W] != am_r
    print(f"case {case} T {T}: argmax mismatches {int(mism.sum())} of {mism.numel()}")
    assert float(mism.float().mean()) < 1e-4
    if mism.any():                             # and only where the two rows are equal to fp32 rounding
        gap = (z_r[:, :, 1::2] - z_r[:, :, 0::2]).abs()[mism]
        assert float(gap.max()) < 1e-5 * float(z_r.abs().max())
    # ---- stats_part: the next block's LayerNorm statistics against fp64 and against a sweep of the stored plane
    stats_swept, stats_fused = torch.empty((B, 64, 2), device=dev), torch.empty((B, 64, 2), device=dev)
    _hip.call("mx_plane_stats", _hip.ptr(p), _hip.ptr(sl_out), B, 64, Hp, W, 1e-5, _hip.ptr(stats_swept), st)
    _hip.call("mx_plane_stats_finish", _hip.ptr(st_part), _hip.ptr(b_d), _hip.ptr(sl_out), B, 64, Hp, W, 1e-5,
              _hip.ptr(stats_fused), st)
    y_r = torch.where(p_r > 0, p_r, sl_out.cpu().double().view(1, 64, 1, 1) * p_r)
    mean_r, var_r = y_r.mean(dim=(2, 3)), y_r.var(dim=(2, 3), unbiased=False)
    assert float(((stats_fused[..., 0].cpu().double() - mean_r).abs() / var_r.sqrt()).max()) < 2e-6
    assert float((stats_fused[..., 1].cpu().double() * (var_r + 1e-5).sqrt() - 1).abs().max()) < 2e-6
    assert float((stats_fused - stats_swept).abs().max() / stats_swept.abs().max()) < 2e-6
    # ---- the optional outputs change nothing else
    p2 = torch.full_like(p, float("nan"))
    amax2 = torch.full_like(amax, 255)
    _hip.call("mx_conv_block_fwd_f16", _hip.ptr(x_hi), _hip.ptr(x_lo), _hip.ptr(w_hi), _hip.ptr(w_lo), _hip.ptr(b_d),
              B, H, W, T, _hip.ptr(p2), _hip.ptr(amax2), None, None, st)
    assert torch.equal(p2, p) and torch.equal(amax2, amax)
    if identity_ln:
        # the exact-fp32 kernel on the same input
        wt = am._pack(w.to(dev), 0)
        p32 = torch.empty_like(p)
        amax32 = torch.empty_like(amax)
        _hip.call("mx_conv_block_fwd", _hip.ptr(x_d), _hip.ptr(stats), _hip.ptr(sl_d), _hip.ptr(wt), _hip.ptr(b_d),
                  B, 64, H, W, T, 0, _hip.ptr(p32), _hip.ptr(amax32), st)
        err32 = rel(p[..., :W], p32[..., :W])
        print(f"case {case} T {T}: against the fp32 kernel {err32:.3g} of the maximum")
        assert err32 < 1e-5
        assert float((amax[..., :W] != amax32[..., :W]).float().mean()) < 1e-4

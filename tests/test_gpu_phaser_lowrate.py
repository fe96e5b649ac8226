"""GPU: the phaser's LFO at a low rate -- mx_phaser_mod_expand / mx_phaser_dmod_gather (csrc/phaser_lr.hip),
fx.phaser_forward_stash_lr / fx.phaser_backward_lr and fx.PhaserModule(.., mod_sig_low_rate=True).

1. expand: bit for bit against util.linear_interpolate_last_dim(mod, N) (mx_interp_linear: the same interp_tap /
   interp_combine of csrc/common.h) indexed at clamp(4 g - lead, 0, N - 1); 0.5 beyond lead + N; per-row leads that differ
   within the batch; a destination wider than the row keeps its padding.
2. gather: against the fp64 helper (tests/helpers/phaser_lr64.py).  Gate: the sums are fp64 and every point is cast to fp32
   once, so the error is one fp32 rounding of a value no larger than max |dmod_lr|: 6e-8 of max |dmod_lr| (2^-24 = 5.96e-8;
   the gate of test_reduction_is_one_cast_from_the_full_rate_path).  Two runs are torch.equal.
3. end to end: forward_stash_lr + backward_lr against phaser_adjoint64 followed by gather64, at the output-clip decisions
   the stash forward took (as tests/test_gpu_phaser_grad.py compares) and at the osc row the scan read.  B = 8, N = 4096
   behind a lead of 512, n_mod = 41, |feedback| <= 0.7.  Gates: GATES["dmod_lo"], ["dx_lo"], ["param_lo"] of
   tests/test_gpu_phaser_grad.py, imported.
4. PhaserModule.apply_effect(mod_sig_low_rate=True): forward bit-identical to the default path fed the expanded row;
   backward fills x.grad, mod_sig.grad at its own rate and the four parameter gradients.

Shapes (N, n_mod, lead): those of tests/test_phaser_lr64.py plus (2047, 9, 0), (2048, 2048, 1), (2049, 9, 2) around the
256-group tile of the expand, and (22272, 88, 441), the step's shape."""
import numpy as np
import pytest
import torch

from tests.helpers import phaser_adjoint64 as pa
from tests.helpers.phaser_lr64 import expand64, gather64
from tests.test_gpu_phaser_grad import GATES, SR, audio_np, dev_params, gpu_decisions, normwise, reference, ulp_edges

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 0), (4, 2, 0), (5, 2, 3), (37, 5, 6), (64, 64, 1), (2047, 9, 0), (2048, 2048, 1), (2049, 9, 2),
          (22272, 88, 441)]


def leads_of(lead):
    """per-row leads that differ within the batch (the first row has the shape's own)"""
    return [lead, 0, lead + 3, lead + 1, 2 * lead + 6]


@pytest.mark.parametrize("N,n_mod,lead", SHAPES)
def test_expand_is_the_resampled_row_bit_for_bit(dev, N, n_mod, lead):
    from mod_extraction_amd import fx
    from mod_extraction_amd.util import linear_interpolate_last_dim
    leads = leads_of(lead)
    B, W = len(leads), N + max(leads) + 5
    ng = (W + 3) // 4
    mod = torch.rand(B, n_mod, device=dev, generator=torch.Generator(device=dev).manual_seed(N + n_mod))
    lead_t = torch.tensor(leads, device=dev, dtype=torch.int32)
    got = fx.phaser_mod_expand(mod, lead_t, N, W)
    assert got.shape == (B, ng)
    up = linear_interpolate_last_dim(mod, N, align_corners=True)
    g = torch.arange(ng, device=dev)[None, :]
    idx = (4 * g - lead_t[:, None].long()).clamp(0, N - 1)
    valid = g < (lead_t[:, None].long() + N + 3) // 4
    want = torch.where(valid, up.gather(1, idx), torch.full_like(got, 0.5))
    assert (~valid).any() and torch.equal(got, want)
    # within one fp32 ulp of the [0, 1] range of the fp64 definition (information: the bit comparison above is the test)
    e = float(np.abs(got.cpu().numpy() - expand64(mod.cpu().numpy(), leads, N, W)).max())
    print(f"expand {(N, n_mod, lead)}: max |mod_g - fp64| = {e:.3e}")
    assert e <= 1.2e-7
    # lead = None is lead 0; a wider destination keeps its padding
    wide = torch.full((B, ng + 3), 7.0, device=dev)
    fx.phaser_mod_expand(mod, None, N, W, out=wide)
    assert (wide[:, ng:] == 7.0).all()
    assert torch.equal(wide[:, :ng], fx.phaser_mod_expand(mod, torch.zeros(B, device=dev, dtype=torch.int32), N, W))
    assert torch.equal(wide[1, :ng], got[1])                                   # the row whose lead is 0


@pytest.mark.parametrize("N,n_mod,lead", SHAPES)
def test_gather_is_one_cast_from_fp64(dev, N, n_mod, lead):
    from mod_extraction_amd import fx
    leads = leads_of(lead)
    B, W = len(leads), N + max(leads) + 5
    ng = (W + 3) // 4
    buf = torch.randn(B, ng + 3, device=dev, generator=torch.Generator(device=dev).manual_seed(7 * N + n_mod))
    d = buf[:, :ng]                                                            # a row stride longer than the row
    lead_t = torch.tensor(leads, device=dev, dtype=torch.int32)
    got = fx.phaser_dmod_gather(d, lead_t, N, n_mod)
    assert got.shape == (B, n_mod) and torch.equal(got, fx.phaser_dmod_gather(d, lead_t, N, n_mod))
    ref = gather64(d.cpu().numpy(), leads, N, n_mod)
    e = normwise(got.cpu().numpy(), ref)
    print(f"gather {(N, n_mod, lead)}: max |dmod_lr - fp64| / max |fp64| = {e:.3e}")
    assert e < 6e-8
    # the transpose identity on the device results: <expand(m) - expand(0), d> == <m, gather(d)>
    m = torch.rand(B, n_mod, device=dev)
    lin = fx.phaser_mod_expand(m, lead_t, N, W).double() - fx.phaser_mod_expand(torch.zeros_like(m), lead_t, N, W).double()
    lhs, rhs = float((lin * d.double()).sum()), float((m.double() * got.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * float((lin.abs() * d.double().abs()).sum() + 1e-30), (lhs, rhs)


def test_end_to_end_matches_fp64(dev):
    from mod_extraction_amd import fx
    B, lead, N, n_mod = 8, 512, 4096, 41
    T = lead + N
    params = {"centre_frequency_hz": np.asarray([70.0, 440.0, 1300.0, 5000.0, 440.0, 2000.0, 800.0, 18000.0], np.float32),
              "feedback": np.asarray([-0.7, 0.0, 0.25, 0.7, 0.5, -0.5, 0.7, 0.3], np.float32),
              "depth": np.asarray([0.2, 1.0, 1.0, 0.2, 0.8, 1.0, 0.5, 1.0], np.float32),
              "mix": np.asarray([0.2, 1.0, 0.7, 1.0, 0.5, 1.0, 0.2, 0.8], np.float32)}
    x_np = audio_np(B, T, 71, 0.9)
    g = np.random.default_rng(72)
    k = np.linspace(0.0, 1.0, n_mod)[None, :]
    mod_np = (0.5 + 0.5 * np.sin(2 * np.pi * (g.uniform(1.0, 3.0, (B, 1)) * k + g.uniform(0, 1, (B, 1))))).astype(np.float32)
    x, mod, p = torch.tensor(x_np, device=dev), torch.tensor(mod_np, device=dev), dev_params(dev, params)
    lead_t = torch.full((B,), lead, device=dev, dtype=torch.int32)
    dy = torch.randn(B, N, device=dev, generator=torch.Generator(device=dev).manual_seed(73))
    y, st, mod_g = fx.phaser_forward_stash_lr(x, p, lead_t, SR, N, mod)
    dx, dmod_lr, grads = fx.phaser_backward_lr(dy, x, st, p, lead_t, SR, N, n_mod)
    assert dx.shape == (B, T) and dmod_lr.shape == (B, n_mod) and set(grads) == set(pa.PARAMS)
    # the osc row the scan read: 1 - 2 mod_g in fp32, from the expand's own output
    mg = mod_g.cpu().numpy()
    assert mg.shape == (B, (T + 3) // 4)
    assert np.abs(mg - expand64(mod_np, [lead] * B, N, T)).max() <= 1.2e-7
    osc = (np.float32(1.0) - np.float32(2.0) * mg).astype(np.float32)
    ref, recompute = reference(x_np, osc, params, lead, dy.cpu().numpy(), with_recompute=True)
    near_m, near_p = ulp_edges(ref)
    clipped, clamped = (~ref["pass_m"]).mean(), (~ref["inside"]).mean()
    print(f"end to end: {clipped:.4f} of the samples clipped, {clamped:.4f} of the groups clamped; within 1 ulp of an edge: "
          f"{int(near_m.sum())} samples, {int(near_p.sum())} groups")
    assert clipped > 0 and clamped > 0 and int(near_p.sum()) == 0
    y32 = ref["fwd32"]["y"][:, lead:]
    e_fwd = float(np.abs(y.cpu().numpy() - y32).max() / np.abs(y32).max())
    print(f"end to end: forward {e_fwd:.3e}")
    assert e_fwd < 1e-5
    mine = gpu_decisions(st, T, T)
    flips = int((mine != ref["pass_m"]).sum())
    print(f"end to end: {flips} output-clip decisions differ between the scan forward and the sequential fp32 forward")
    if flips:
        ref = recompute(mine)
    keep = ~near_m
    out = {"dx_lo": normwise(np.where(keep, dx.cpu().numpy(), 0.0), np.where(keep, ref["dx"], 0.0)),
           "dmod_lo": normwise(dmod_lr.cpu().numpy(), gather64(ref["dmod"], [lead] * B, N, n_mod))}
    for name in pa.PARAMS:
        out[name] = normwise(grads[name].cpu().numpy(), ref[name])
    print("end to end", {k_: f"{v:.2e}" for k_, v in out.items()})
    assert out["dx_lo"] < GATES["dx_lo"]
    assert out["dmod_lo"] < GATES["dmod_lo"]
    for name in pa.PARAMS:
        assert out[name] < GATES["param_lo"], name
    # dmod alone (what the training step asks for): the same bits, no dx, no parameter sums
    dx2, dmod2, g2 = fx.phaser_backward_lr(dy, x, st, p, lead_t, SR, N, n_mod, need_dx=False, params_wanted=())
    assert dx2 is None and g2 == {} and torch.equal(dmod2, dmod_lr)


def test_module_low_rate_path(dev):
    from mod_extraction_amd import fx
    B, n_ch, W, n_mod = 3, 2, 4411, 23
    leads = torch.tensor([0, 221, 441], device=dev)
    n = W - 441
    m = fx.PhaserModule(SR)
    x = torch.tensor(audio_np(B * n_ch, W, 81, 0.8), device=dev).view(B, n_ch, W).requires_grad_(True)
    k = torch.linspace(0.0, 1.0, n_mod, device=dev)
    mod = (0.5 + 0.4 * torch.sin(2 * np.pi * (1.5 * k[None, :] + torch.arange(B, device=dev)[:, None] / B))).requires_grad_(True)
    ps = {"depth": torch.tensor([0.8, 0.5, 1.0], device=dev, requires_grad=True),
          "centre_frequency_hz": torch.tensor([440.0, 1300.0, 3000.0], device=dev, requires_grad=True),
          "feedback": torch.tensor([0.3, -0.7, 0.6], device=dev, requires_grad=True),
          "mix": torch.tensor([0.75, 1.0, 0.5], device=dev, requires_grad=True)}
    y = m.apply_effect(x, mod_sig=mod, lead=leads, mod_sig_low_rate=True, **ps)
    assert y.shape == (B, n_ch, n) and y.grad_fn is not None
    # the default path fed the expanded row
    mod_g = fx.phaser_mod_expand(mod.detach(), leads.to(torch.int32), n, W)
    detached = {k_: v.detach() for k_, v in ps.items()}
    y0 = m(x.detach(), mod_sig=mod_g, lead=leads, **detached)
    assert torch.equal(y.detach(), y0)
    assert torch.equal(m(x.detach(), mod_sig=mod.detach(), lead=leads, mod_sig_low_rate=True, **detached), y0)
    assert torch.equal(m(x.detach(), mod_sig=mod.detach().unsqueeze(1), lead=leads, mod_sig_low_rate=True, **detached), y0)
    dy = torch.randn_like(y)
    (y * dy).sum().backward()
    assert x.grad.shape == x.shape and mod.grad.shape == (B, n_mod)
    for name, t in [("x", x), ("mod", mod)] + list(ps.items()):
        assert t.grad is not None and torch.isfinite(t.grad).all() and float(t.grad.abs().sum()) > 0, name
    # the low-rate gradient is the gather of the default path's group-rate gradient (channels summed by autograd)
    mg = mod_g.clone().requires_grad_(True)
    (m.apply_effect(x.detach(), mod_sig=mg, lead=leads, **detached) * dy).sum().backward()
    want = fx.phaser_dmod_gather(mg.grad, leads.to(torch.int32), n, n_mod)
    e = normwise(mod.grad.cpu().numpy(), want.cpu().numpy())
    print(f"module: low-rate dmod against the gather of the default path's: {e:.3e}")
    assert e < 1e-6            # two fp32 roundings apart (the channels are summed before / after the gather)
    with torch.no_grad():
        assert m.apply_effect(x, mod_sig=mod, lead=leads, mod_sig_low_rate=True).grad_fn is None
    with pytest.raises(AssertionError):
        m.apply_effect(x, mod_sig=torch.rand(B, n + 1, device=dev), lead=leads, mod_sig_low_rate=True)

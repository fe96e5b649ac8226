"""GPU: the flanger / chorus adjoint for a LOW-RATE LFO row (mx_flanger_fwd_stash with n_mod < N + mx_flanger_bwd_lr) against
the fp64 reference of tests/helpers/flanger_adjoint64_lr.py.

Gates.  dx, the five parameter gradients and dmod at feedback 0.99 carry the gates of tests/test_gpu_flanger_grad.py
(dx 2e-6 at feedback <= 0.7 and 1e-5 at 0.99, parameters 1e-5, all norm-wise over a batch); the low-rate dmod (B, n_mod) at
feedback <= 0.7 carries that file's 3e-6.  The new reduction on its own (test_reduction_is_one_cast_from_the_full_rate_path)
is gated by the number format: the kernel gathers the SAME fp32 per-sample values with the SAME fp32 weights as the host
does from the full-rate path's dmod, in fp64 (ordering noise ~n 2^-53), and rounds once, so a point differs by at most
2^-24 of its value = 5.96e-8 < 6e-8 norm-wise.  Every gate reports its measured value."""
import math

import numpy as np
import pytest
import torch

from tests.helpers.flanger_adjoint64_lr import flanger_adjoint64_lr, interp_transpose64, upsample32
from tests.test_gpu_flanger_grad import DELAYS, PARAMS, SHAPES, SR, audio, grid_consts, lfos, normwise, np_consts

pytestmark = pytest.mark.gpu


def lfos_lr(dev, B, n_mod, N, seed, shapes=SHAPES):
    """B low-rate LFO rows of n_mod points spanning N samples (the data path's label: lfo_sr = sr * n_mod / N)."""
    from mod_extraction_amd import modulations as amod
    g = np.random.default_rng(seed)
    rows = []
    for i in range(B):
        ex = 2.0 if i % 4 == 3 else 1.0
        rows.append(amod.make_mod_signal(n_mod, SR * n_mod / N, float(g.uniform(0.5, 4.0)), float(g.uniform(0, 2 * math.pi)),
                                         shapes[i % len(shapes)], ex, device=dev))
    return torch.stack(rows).contiguous()


def fwd_ref(x, mod, consts, M, rows=None, out=None):
    """mx_flanger_fwd and its per-sample LFO."""
    from mod_extraction_amd import fx
    B, N = x.shape
    md = torch.full((B,), M, device=x.device, dtype=torch.int32)
    up = torch.zeros((B, N), device=x.device) if mod.size(1) != N else None
    y = fx.flanger_forward(x, mod, consts, md, M, rows=rows, out=out, mod_up=up)
    return y, (up if up is not None else mod)


def run_lr(x, mod, consts, M, dy, rows=None, **kw):
    from mod_extraction_amd import fx
    md = torch.full((x.size(0),), M, device=x.device, dtype=torch.int32)
    y, st = fx.flanger_forward_stash(x, mod, consts, md, M, rows=rows)
    dx, dmod, g = fx.flanger_backward(dy, x, mod, st, consts, md, M, rows=rows, **kw)
    return y, st, dx, dmod, g


@pytest.mark.parametrize("name,N,n_mod", [("flanger", 88200, 882), ("flanger", 88200, 345), ("chorus", 88200, 345),
                                          ("chorus", 88200, 88200), ("flanger", 50001, 500), ("chorus", 50001, 345),
                                          ("flanger", 50001, 50001)])
def test_stash_forward_equals_renderer(dev, name, N, n_mod):
    """y of the low-rate stash forward is mx_flanger_fwd's, bit for bit: dense rows, a rows subset, strided rows."""
    from mod_extraction_amd import fx
    B = 8
    mod = lfos_lr(dev, B, n_mod, N, 7 + n_mod % 13)
    consts, M, _ = grid_consts(dev, B, mod, DELAYS[name])
    xx = audio(dev, 2 * B, N, 8).view(B, 2, N)
    md = torch.full((B,), M, device=dev, dtype=torch.int32)
    for x in (xx[:, 0].contiguous(), xx[:, 1]):                                # dense, then one channel of (B, 2, N)
        y0, _ = fwd_ref(x, mod, consts, M)
        y, st = fx.flanger_forward_stash(x, mod, consts, md, M)
        assert torch.equal(y, y0)
        assert torch.isfinite(st).all()
    rows = torch.tensor([6, 1, 4], device=dev, dtype=torch.int32)
    x = xx[:, 0].contiguous()
    y0, _ = fwd_ref(x, mod, consts, M, rows=rows, out=torch.full((B, N), 7.0, device=dev))
    y, _ = fx.flanger_forward_stash(x, mod, consts, md, M, rows=rows, out=torch.full((B, N), 7.0, device=dev))
    assert torch.equal(y, y0) and (y[[0, 2, 3, 5, 7]] == 7.0).all()


def check_lr_against_fp64(x, mod, consts, M, dy, mod_up, y, dx, dmod, g, fbs, rows=None):
    sel = np.arange(x.shape[0]) if rows is None else np.asarray(rows)
    xs, ms, dys, ups = (t.cpu().numpy()[sel] for t in (x, mod, dy, mod_up))
    c = {k: v[sel] for k, v in np_consts(consts).items()}
    assert np.array_equal(upsample32(ms, xs.shape[1]), ups)                   # the helper's resampling is the kernel's
    ref = flanger_adjoint64_lr(xs, ms, c, M, dys, mod_full=ups)
    assert np.array_equal(y.cpu().numpy()[sel], ref["fwd"]["y32"])           # the forward is the fp32 reference
    assert dmod.shape == mod.shape
    lo, hi = fbs[sel] <= 0.7, fbs[sel] > 0.7
    out = {}
    if lo.any():
        out["dx_lo"] = e = normwise(dx.cpu().numpy()[sel], ref["dx"], lo)
        assert e < 2e-6
        out["dmod_lo"] = e = normwise(dmod.cpu().numpy()[sel], ref["dmod"], lo)
        assert e < 3e-6
    if hi.any():
        out["dx_hi"] = e = normwise(dx.cpu().numpy()[sel], ref["dx"], hi)
        assert e < 1e-5
        out["dmod_hi"] = e = normwise(dmod.cpu().numpy()[sel], ref["dmod"], hi)
        assert e < 1e-5
    for k in PARAMS:
        out[k] = e = normwise(g[k].cpu().numpy()[sel], ref[k], np.ones(len(sel), bool))
        assert e < 1e-5, k
    return out


@pytest.mark.parametrize("name,N,n_mod", [("flanger", 88200, 882), ("flanger", 88200, 345), ("chorus", 88200, 345),
                                          ("eval", 50001, 500)])
def test_grid_matches_fp64(dev, name, N, n_mod):
    B = 24
    mod = lfos_lr(dev, B, n_mod, N, 10 + len(name), SHAPES + ["saw", "saw"])
    consts, M, fbs = grid_consts(dev, B, mod, DELAYS[name])
    x = audio(dev, B, N, 20 + len(name))
    dy = torch.randn(B, N, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    _, up = fwd_ref(x, mod, consts, M)
    y, st, dx, dmod, g = run_lr(x, mod, consts, M, dy)
    print(name, N, n_mod, check_lr_against_fp64(x, mod, consts, M, dy, up, y, dx, dmod, g, fbs))


def test_long_clips_rows_subset_and_strided(dev):
    """4 s clips with n_mod = 690 (the extractor's frame rate); a rows subset leaves the other rows
    untouched; x / dy / dx as one channel of a (B, 2, N) tensor."""
    from mod_extraction_amd import fx
    B, N, n_mod = 6, 176400, 690
    mod = lfos_lr(dev, B, n_mod, N, 31)
    consts, M, fbs = grid_consts(dev, B, mod, DELAYS["flanger"])
    xx = audio(dev, 2 * B, N, 32).view(B, 2, N)
    x = xx[:, 1]
    dy = torch.randn(B, 2, N, device=dev, generator=torch.Generator(device=dev).manual_seed(4))[:, 0]
    rows = torch.tensor([5, 0, 3], device=dev, dtype=torch.int32)
    md = torch.full((B,), M, device=dev, dtype=torch.int32)
    _, up = fwd_ref(x, mod, consts, M)
    y, st = fx.flanger_forward_stash(x, mod, consts, md, M, rows=rows, out=torch.full((B, N), 7.0, device=dev))
    dxx = torch.full((B, 2, N), 7.0, device=dev)
    dmod = torch.full((B, n_mod), 7.0, device=dev)
    dx, dmod, g = fx.flanger_backward(dy, x, mod, st, consts, md, M, rows=rows, dx=dxx[:, 1], dmod=dmod)
    untouched = [1, 2, 4]
    assert (y[untouched] == 7.0).all() and (dx[untouched] == 7.0).all() and (dmod[untouched] == 7.0).all()
    assert (dxx[:, 0] == 7.0).all()
    assert all((g[k][untouched] == 0).all() for k in PARAMS)
    print(check_lr_against_fp64(x, mod, consts, M, dy, up, y, dx, dmod, g, fbs, rows=[5, 0, 3]))
    # optional outputs: NULL dx, one parameter
    _, dmod2, g2 = fx.flanger_backward(dy, x, mod, st, consts, md, M, rows=rows, need_dx=False, params=("mix",))
    assert torch.equal(dmod2[[5, 0, 3]], dmod[[5, 0, 3]]) and torch.equal(g2["mix"], g["mix"]) and set(g2) == {"mix"}


@pytest.mark.parametrize("name,N,n_mod", [("flanger", 88200, 345), ("chorus", 50001, 500)])
def test_reduction_is_one_cast_from_the_full_rate_path(dev, name, N, n_mod):
    """The new reduction alone: the existing full-rate path on the forward's own per-sample LFO gives the fp32 per-sample
    dmod; reduced on the host in fp64 with the transposed resampling it is the low-rate kernel's dmod up to ONE fp32 cast
    per point.  dx and the parameter gradients of the two paths are the same bits."""
    from mod_extraction_amd import fx
    B = 24
    mod = lfos_lr(dev, B, n_mod, N, 40, SHAPES + ["saw", "saw"])
    consts, M, _ = grid_consts(dev, B, mod, DELAYS[name])
    x = audio(dev, B, N, 41)
    dy = torch.randn(B, N, device=dev, generator=torch.Generator(device=dev).manual_seed(6))
    md = torch.full((B,), M, device=dev, dtype=torch.int32)
    _, up = fwd_ref(x, mod, consts, M)
    y_f, st_f = fx.flanger_forward_stash(x, up, consts, md, M)
    dx_f, dmod_f, g_f = fx.flanger_backward(dy, x, up, st_f, consts, md, M)
    y, st, dx, dmod, g = run_lr(x, mod, consts, M, dy)
    assert torch.equal(y, y_f) and torch.equal(st, st_f) and torch.equal(dx, dx_f)
    assert all(torch.equal(g[k], g_f[k]) for k in PARAMS)
    want = interp_transpose64(dmod_f.cpu().numpy(), n_mod)
    got = dmod.cpu().numpy().astype(np.float64)
    err = normwise(got, want, slice(None))
    print(name, "reduction vs host fp64 gather", err)
    assert err < 6e-8
    assert (np.abs(got - want) <= 2.0 ** -24 * np.abs(want) + 1e-12 * np.abs(want).max()).all()   # per point: one cast


def test_backward_is_deterministic(dev):
    B, N, n_mod = 24, 88200, 345
    mod = lfos_lr(dev, B, n_mod, N, 51, ["saw", "cos", "tri"])
    consts, M, _ = grid_consts(dev, B, mod, DELAYS["flanger"])
    x = audio(dev, B, N, 52)
    dy = torch.randn(B, N, device=dev)
    _, _, dx1, dm1, g1 = run_lr(x, mod, consts, M, dy)
    _, _, dx2, dm2, g2 = run_lr(x, mod, consts, M, dy)
    assert torch.equal(dx1, dx2) and torch.equal(dm1, dm2)
    assert all(torch.equal(g1[k], g2[k]) for k in PARAMS)


def test_lds_budget_and_arguments(dev):
    """The LFO row counts against the LDS budget of both launchers; n_mod > N is an argument error."""
    from mod_extraction_amd import _hip, fx
    B, N = 2, 44100
    M = 34000
    consts = fx.derive_clip_constants(B, dev, 0, M, 0.3, 1.0, 1.0, 0.8, 0.5)
    md = torch.full((B,), M, device=dev, dtype=torch.int32)
    x = audio(dev, B, N, 1)
    with pytest.raises(_hip.HipLibraryError, match="UNSUPPORTED"):
        fx.flanger_forward_stash(x, torch.rand(B, 1000, device=dev), consts, md, M)      # 34000 + 1000 > 34784
    st = torch.zeros(B, N, device=dev)
    with pytest.raises(_hip.HipLibraryError, match="UNSUPPORTED"):
        fx.flanger_backward(x, x, torch.rand(B, 1000, device=dev), st, consts, md, M)
    y, st = fx.flanger_forward_stash(x, torch.rand(B, 700, device=dev), consts, md, M)   # fits
    assert torch.isfinite(y).all()


def test_apply_effect_low_rate_and_full_rate(dev):
    """apply_effect with a low-rate mod_sig that requires grad returns mod_sig.grad at the low rate (against fp64, two
    channels sharing the row); a full-rate call still takes mx_flanger_bwd: its gradients are those of the launch itself and
    of mx_flanger_bwd_lr with n_mod == N, bit for bit."""
    from mod_extraction_amd import fx
    B, N, n_mod = 3, 44100, 345
    m = fx.MonoFlangerChorusModule(B, 2, N, SR, 1.0, 10.0)
    x = audio(dev, 2 * B, N, 61).view(B, 2, N).requires_grad_(True)
    mod = lfos_lr(dev, B, n_mod, N, 62).requires_grad_(True)
    fb = torch.tensor([0.3, 0.7, 0.5], device=dev, requires_grad=True)
    y = m.apply_effect(x, mod, fb, 0.5, 1.0, 0.8, 0.75)
    assert y.grad_fn is not None and torch.equal(y.detach(), m(x.detach(), mod.detach(), fb.detach(), 0.5, 1.0, 0.8, 0.75))
    dy = torch.randn_like(y)
    (y * dy).sum().backward()
    assert mod.grad.shape == (B, n_mod) and x.grad.shape == x.shape
    c = fx.derive_clip_constants(B, dev, m.max_min_delay_samples, m.max_lfo_delay_samples, fb.detach(), 0.5, 1.0, 0.8, 0.75)
    c = {k: v.repeat_interleave(2).cpu().numpy() for k, v in c.items()}
    rows_mod = mod.detach().repeat_interleave(2, 0).cpu().numpy()
    ref = flanger_adjoint64_lr(x.detach().reshape(2 * B, N).cpu().numpy(), rows_mod, c, m.max_delay_samples,
                               dy.reshape(2 * B, N).cpu().numpy())
    assert normwise(x.grad.reshape(2 * B, N).cpu().numpy(), ref["dx"], slice(None)) < 2e-6
    assert normwise(mod.grad.cpu().numpy(), ref["dmod"].reshape(B, 2, n_mod).sum(1), slice(None)) < 3e-6
    assert normwise(fb.grad.cpu().numpy(), ref["feedback"].reshape(B, 2).sum(1), slice(None)) < 1e-5
    # full rate: unchanged route
    m1 = fx.MonoFlangerChorusModule(B, 1, N, SR, 1.0, 10.0)
    x1 = audio(dev, B, N, 63).unsqueeze(1).requires_grad_(True)
    full = lfos(dev, B, N, 64).requires_grad_(True)
    y1 = m1.apply_effect(x1, full, 0.7, 0.5, 1.0, 0.8, 0.75)
    dy1 = torch.randn_like(y1)
    (y1 * dy1).sum().backward()
    consts = fx.derive_clip_constants(B, dev, m1.max_min_delay_samples, m1.max_lfo_delay_samples, 0.7, 0.5, 1.0, 0.8, 0.75)
    md = torch.full((B,), m1.max_delay_samples, device=dev, dtype=torch.int32)
    xr, dyr = x1.detach()[:, 0], dy1[:, 0].contiguous()
    y0, st = fx.flanger_forward_stash(xr, full.detach(), consts, md, m1.max_delay_samples)
    dx0, dmod0, g0 = fx.flanger_backward(dyr, xr, full.detach(), st, consts, md, m1.max_delay_samples)
    assert torch.equal(y1.detach()[:, 0], y0) and torch.equal(y0, fwd_ref(xr, full.detach(), consts, m1.max_delay_samples)[0])
    assert torch.equal(x1.grad[:, 0], dx0) and torch.equal(full.grad, dmod0)
    from mod_extraction_amd import _hip
    dx2, dmod2 = torch.empty_like(dx0), torch.empty_like(dmod0)
    g2 = {k: torch.zeros(B, device=dev, dtype=torch.float64) for k in PARAMS}
    ws = torch.empty(B, N, device=dev)
    _hip.call("mx_flanger_bwd_lr", dyr.data_ptr(), N, xr.data_ptr(), xr.stride(0), _hip.ptr(full.detach()), N, _hip.ptr(st),
              *[_hip.ptr(consts[k]) for k in ("lfo_scale", "min_delay", "feedback", "depth", "mix", "one_minus_mix")],
              _hip.ptr(md), m1.max_delay_samples, None, 0, B, N, _hip.ptr(ws), _hip.ptr(dx2), N, _hip.ptr(dmod2), N,
              *[_hip.ptr(g2[k]) for k in PARAMS], _hip.stream())
    assert torch.equal(dx2, dx0) and torch.equal(dmod2, dmod0) and all(torch.equal(g2[k], g0[k]) for k in PARAMS)

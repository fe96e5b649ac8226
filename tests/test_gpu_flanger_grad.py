"""GPU: the differentiable flanger / chorus (mx_flanger_fwd_stash + mx_flanger_bwd, fx.MonoFlangerChorusModule.apply_effect)
against the fp64 explicit adjoint of tests/helpers/flanger_adjoint64.py.

Grid: the delay settings of train_lfo_flanger.yml (1 / 10 ms), eval_lfo*.yml (1 / 4 ms) and the chorus (10 / 30 ms);
feedback {0, 0.3, 0.7, 0.99} x mix {0.25, 1} x min_delay_width {0, 0.5, 1}; the six continuous LFO shapes, exp 2 and saw
(steep delay slopes: the run-splitting case of the adjoint's lock-steps); input gain 1.6 (the output clips).

Gates, about 10x above the worst values measured on an MI355X (in brackets): dx, dmod max|g - g64| / max|g64| over a
batch <= 2e-6 at feedback <= 0.7 [1.5e-7] and <= 1e-5 at 0.99 [7e-7]; the fp64-summed parameter gradients the same
norm-wise over a batch <= 1e-5 [8.6e-7].  Every gate reports its measured value."""
import math

import numpy as np
import pytest
import torch

from tests.helpers.flanger_adjoint64 import flanger_adjoint64

pytestmark = pytest.mark.gpu
SR = 44100.0
DELAYS = {"flanger": (1.0, 10.0), "eval": (1.0, 4.0), "chorus": (10.0, 30.0)}
SHAPES = ["cos", "rect_cos", "inv_rect_cos", "tri", "saw", "rsaw"]
PARAMS = ("lfo_scale", "min_delay", "feedback", "depth", "mix")


def lfos(dev, B, N, seed, shapes=SHAPES):
    from mod_extraction_amd import modulations as amod
    g = np.random.default_rng(seed)
    rows = []
    for i in range(B):
        shape = shapes[i % len(shapes)]
        ex = 2.0 if i % 4 == 3 else 1.0
        rows.append(amod.make_mod_signal(N, SR, float(g.uniform(0.5, 4.0)), float(g.uniform(0, 2 * math.pi)), shape, ex,
                                         device=dev))
    return torch.stack(rows)


def audio(dev, B, N, seed, gain=1.6):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = torch.arange(N) / SR
    x = 0.5 * torch.sin(2 * math.pi * 220.0 * t)[None, :] + (torch.rand(B, N, generator=g) - 0.5) * 0.8
    return (gain * x).float().to(dev)


def run(dev, x, mod, consts, M, dy, rows=None):
    from mod_extraction_amd import fx
    B = x.size(0)
    md = torch.full((B,), M, device=dev, dtype=torch.int32)
    y, st = fx.flanger_forward_stash(x, mod, consts, md, M, rows=rows)
    dx, dmod, g = fx.flanger_backward(dy, x, mod, st, consts, md, M, rows=rows)
    return y, st, dx, dmod, g


def np_consts(consts):
    return {k: v.cpu().numpy() for k, v in consts.items()}


def grid_consts(dev, B, mods, delays):
    from mod_extraction_amd import fx
    combos = [(fb, mx, mdw) for fb in (0.0, 0.3, 0.7, 0.99) for mx in (0.25, 1.0) for mdw in (0.0, 0.5, 1.0)]
    fb, mx, mdw = (torch.tensor([c[i] for c in combos][:B], device=dev) for i in range(3))
    M_min, M_lfo = (fx.delay_samples(ms, SR) for ms in delays)
    consts = fx.derive_clip_constants(B, dev, M_min, M_lfo, fb, mdw, torch.ones(B, device=dev),
                                      torch.full((B,), 0.8, device=dev), mx)
    return consts, M_min + M_lfo, fb.cpu().numpy()


def normwise(a, b, sel):
    a, b = np.asarray(a, np.float64)[sel], np.asarray(b, np.float64)[sel]
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def check_against_fp64(x, mod, consts, M, dy, y, dx, dmod, g, fbs, rows=None):
    sel = np.arange(x.shape[0]) if rows is None else np.asarray(rows)
    xs, ms, dys = x.cpu().numpy()[sel], mod.cpu().numpy()[sel], dy.cpu().numpy()[sel]
    c = {k: v[sel] for k, v in np_consts(consts).items()}
    ref = flanger_adjoint64(xs, ms, c, M, dys)
    assert np.array_equal(y.cpu().numpy()[sel], ref["fwd"]["y32"])           # the forward is the fp32 reference
    assert (np.abs(ref["fwd"]["z32"]) > 1).any()
    lo, hi = fbs[sel] <= 0.7, fbs[sel] > 0.7
    out = {}
    for k, t in (("dx", dx), ("dmod", dmod)):
        got = t.cpu().numpy()[sel]
        if lo.any():
            e = normwise(got, ref[k], lo)
            assert e < 2e-6, k
            out[k + "_lo"] = e
        if hi.any():
            e = normwise(got, ref[k], hi)
            assert e < 1e-5, k
            out[k + "_hi"] = e
    for k in PARAMS:
        e = normwise(g[k].cpu().numpy()[sel], ref[k], np.ones(len(sel), bool))
        assert e < 1e-5, k
        out[k] = e
    return out


def test_apply_effect_is_differentiable(dev):
    """Fails without the adjoint: apply_effect on an x that requires grad returns a y with a grad_fn, bit-identical to
    forward(), and y.sum().backward() fills x.grad."""
    from mod_extraction_amd import fx
    B, N = 3, 22050
    m = fx.MonoFlangerChorusModule(B, 1, N, SR, 1.0, 10.0)
    x = audio(dev, B, N, 1).unsqueeze(1).requires_grad_(True)
    mod = lfos(dev, B, N, 2)
    y = m.apply_effect(x, mod, 0.7, 0.5, 1.0, 0.8, 0.75)
    assert y.grad_fn is not None
    assert torch.equal(y.detach(), m(x.detach(), mod, 0.7, 0.5, 1.0, 0.8, 0.75))
    y.sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all() and x.grad.abs().sum() > 0
    with torch.no_grad():                                                     # without grad mode: today's path
        assert m.apply_effect(x, mod, 0.7, 0.5, 1.0, 0.8, 0.75).grad_fn is None


@pytest.mark.parametrize("name", list(DELAYS))
def test_grid_matches_fp64(dev, name):
    B, N = 24, 88200
    mod = lfos(dev, B, N, 10 + len(name), SHAPES + ["saw", "saw"])
    consts, M, fbs = grid_consts(dev, B, mod, DELAYS[name])
    x = audio(dev, B, N, 20 + len(name))
    dy = torch.randn(B, N, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    y, st, dx, dmod, g = run(dev, x, mod, consts, M, dy)
    print(name, check_against_fp64(x, mod, consts, M, dy, y, dx, dmod, g, fbs))


def test_long_clips_and_rows_subset(dev):
    """4 s clips; a rows subset leaves the other rows' outputs untouched."""
    from mod_extraction_amd import fx
    B, N = 6, 176400
    mod = lfos(dev, B, N, 31)
    consts, M, fbs = grid_consts(dev, B, mod, DELAYS["flanger"])
    x = audio(dev, B, N, 32)
    dy = torch.randn(B, N, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    rows = torch.tensor([5, 0, 3], device=dev, dtype=torch.int32)
    md = torch.full((B,), M, device=dev, dtype=torch.int32)
    y = torch.full((B, N), 7.0, device=dev)
    y, st = fx.flanger_forward_stash(x, mod, consts, md, M, rows=rows, out=y)
    dx = torch.full((B, N), 7.0, device=dev)
    dx, dmod, g = fx.flanger_backward(dy, x, mod, st, consts, md, M, rows=rows, dx=dx)
    untouched = [1, 2, 4]
    assert (y[untouched] == 7.0).all() and (dx[untouched] == 7.0).all()
    assert all((g[k][untouched] == 0).all() for k in PARAMS)
    print(check_against_fp64(x, mod, consts, M, dy, y, dx, dmod, g, fbs, rows=[5, 0, 3]))


def test_stash_forward_bit_identical_and_strided(dev):
    """y of the stash forward == mx_flanger_fwd; one channel of a (B, 2, N) tensor as strided x / dx rows; NULL outputs."""
    from mod_extraction_amd import fx
    B, N = 8, 88200
    mod = lfos(dev, B, N, 41)
    consts, M, fbs = grid_consts(dev, B, mod, DELAYS["chorus"])
    xx = audio(dev, 2 * B, N, 42).view(B, 2, N)
    x = xx[:, 1]
    md = torch.full((B,), M, device=dev, dtype=torch.int32)
    y0 = fx.flanger_forward(x.contiguous(), mod, consts, md, M)
    y, st = fx.flanger_forward_stash(x, mod, consts, md, M)
    assert torch.equal(y, y0)
    dy = torch.randn(B, 2, N, device=dev)[:, 0]
    dxx = torch.zeros(B, 2, N, device=dev)
    fx.flanger_backward(dy, x, mod, st, consts, md, M, dx=dxx[:, 1], need_dmod=False)
    dx_ref, dmod_ref, g_ref = fx.flanger_backward(dy.contiguous(), x.contiguous(), mod, st, consts, md, M)
    assert torch.equal(dxx[:, 1], dx_ref) and (dxx[:, 0] == 0).all()
    _, dmod, g = fx.flanger_backward(dy, x, mod, st, consts, md, M, need_dx=False, params=("mix",))
    assert torch.equal(dmod, dmod_ref) and torch.equal(g["mix"], g_ref["mix"]) and set(g) == {"mix"}


def test_backward_is_deterministic(dev):
    B, N = 24, 88200
    mod = lfos(dev, B, N, 51, ["saw", "cos", "tri"])
    consts, M, _ = grid_consts(dev, B, mod, DELAYS["flanger"])
    x = audio(dev, B, N, 52)
    dy = torch.randn(B, N, device=dev)
    _, _, dx1, dm1, g1 = run(dev, x, mod, consts, M, dy)
    _, _, dx2, dm2, g2 = run(dev, x, mod, consts, M, dy)
    assert torch.equal(dx1, dx2) and torch.equal(dm1, dm2)
    assert all(torch.equal(g1[k], g2[k]) for k in PARAMS)


def test_multichannel_and_mixed_params(dev):
    """n_ch = 2 with a shared (B, N) and a per-channel (B, 2, N) mod_sig; float and tensor parameters mixed: the tensor ones
    get (B,) gradients summed over the channels, chain-ruled through derive_clip_constants; the others get None."""
    from mod_extraction_amd import fx
    B, N = 3, 44100
    m = fx.MonoFlangerChorusModule(B, 2, N, SR, 1.0, 10.0)
    for per_channel in (False, True):
        x = audio(dev, 2 * B, N, 61).view(B, 2, N).requires_grad_(True)
        mod = (lfos(dev, 2 * B, N, 62).view(B, 2, N) if per_channel else lfos(dev, B, N, 62)).requires_grad_(True)
        fb = torch.tensor([0.3, 0.7, 0.9], device=dev, requires_grad=True)
        width = torch.tensor([1.0, 0.6, 0.8], device=dev, requires_grad=True)
        mdw = torch.tensor([0.5, 0.0, 1.0], device=dev, requires_grad=True)
        depth = torch.tensor([0.8, 0.5, 1.0], device=dev)                        # a tensor that does not require grad
        y = m.apply_effect(x, mod, fb, mdw, width, depth, 0.75)
        dy = torch.randn_like(y)
        (y * dy).sum().backward()
        assert depth.grad is None
        # fp64 reference, rows = (clip, channel)
        rows_mod = (mod if per_channel else mod.unsqueeze(1).expand(-1, 2, -1)).detach().reshape(2 * B, N)
        c = fx.derive_clip_constants(B, dev, m.max_min_delay_samples, m.max_lfo_delay_samples, fb.detach(), mdw.detach(),
                                     width.detach(), depth, 0.75)
        c = {k: v.repeat_interleave(2).cpu().numpy() for k, v in c.items()}
        ref = flanger_adjoint64(x.detach().reshape(2 * B, N).cpu().numpy(), rows_mod.cpu().numpy(), c,
                                m.max_delay_samples, dy.reshape(2 * B, N).cpu().numpy())
        assert normwise(x.grad.reshape(2 * B, N).cpu().numpy(), ref["dx"], slice(None)) < 2e-6
        dmod_ref = ref["dmod"].reshape(B, 2, N)
        dmod_ref = dmod_ref if per_channel else dmod_ref.sum(1)
        assert normwise(mod.grad.cpu().numpy(), dmod_ref, slice(None)) < 3e-6
        pair = lambda k: ref[k].reshape(B, 2).sum(1)
        expect = {"fb": pair("feedback"), "width": pair("lfo_scale") * m.max_lfo_delay_samples,
                  "mdw": pair("min_delay") * m.max_min_delay_samples}
        for name, t in (("fb", fb), ("width", width), ("mdw", mdw)):
            assert normwise(t.grad.cpu().numpy(), expect[name], slice(None)) < 1e-5, name


def test_full_batch_256x4s(dev):
    """256 clips x 4 s of flanger and chorus rows (two launches); a sampled subset against the fp64 adjoint."""
    B, N = 256, 176400
    for name in ("flanger", "chorus"):
        mod = lfos(dev, B, N, 71)
        consts, M, fbs = grid_consts(dev, 24, mod, DELAYS[name])
        consts = {k: v.repeat(11)[:B].contiguous() for k, v in consts.items()}
        fbs = np.tile(fbs, 11)[:B]
        x = audio(dev, B, N, 72)
        dy = torch.randn(B, N, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
        y, st, dx, dmod, g = run(dev, x, mod, consts, M, dy)
        assert torch.isfinite(dx).all() and torch.isfinite(dmod).all()
        sample = [0, 3, 101, 255] if name == "flanger" else [7, 130]
        print(name, check_against_fp64(x, mod, consts, M, dy, y, dx, dmod, g, fbs, rows=sample))


def test_fit_by_analysis_by_synthesis(dev):
    """End to end.  Setup: 4 clips x 0.5 s of band-limited audio (220-440 Hz sines + 0.2 gain noise-free partials), a
    flanger with 1 ms minimum and 1 ms LFO delay, a cos LFO at 2 Hz built from torch ops at full rate with the phase as a
    learnable parameter.  Targets use feedback 0.5, depth 0.7, phase 1.0 and mix 0.8 (fixed: at unclipped levels y depends
    on mix and depth only through their product, so the pair is not identifiable).  Adam (lr 0.02, decaying to 2e-4 over
    500 steps) on the L1 loss through apply_effect from feedback, depth and phase 0.2 away.  The loss must fall >= 100x and
    every parameter end within 0.02 of its true value."""
    from mod_extraction_amd import fx
    B, N = 4, 22050
    m = fx.MonoFlangerChorusModule(B, 1, N, SR, 1.0, 1.0)
    t = (torch.arange(N, device=dev) / SR).float()
    x = (0.3 * torch.sin(2 * math.pi * 220.0 * t) + 0.2 * torch.sin(2 * math.pi * 330.0 * t + 1.0) +
         0.15 * torch.sin(2 * math.pi * 440.0 * t + 2.0)).expand(B, N).unsqueeze(1).contiguous()
    x = x * torch.linspace(0.8, 1.2, B, device=dev).view(B, 1, 1)
    true = {"fb": 0.5, "depth": 0.7, "phase": 1.0}

    def render(fb, depth, phase):
        mod = (torch.cos(2 * math.pi * 2.0 * t[None, :] + phase[:, None]) + 1.0) / 2.0
        return m.apply_effect(x, mod, fb, 1.0, 1.0, depth, 0.8)

    with torch.no_grad():
        target = render(*(torch.full((B,), true[k], device=dev) for k in ("fb", "depth", "phase")))
    p = {k: torch.full((B,), v - 0.2, device=dev, requires_grad=True) for k, v in true.items()}
    opt = torch.optim.Adam(p.values(), lr=0.02)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.01 ** (1 / 500))
    losses = []
    for _ in range(500):
        opt.zero_grad()
        loss = (render(p["fb"], p["depth"], p["phase"]) - target).abs().mean()
        loss.backward()
        opt.step()
        sched.step()
        with torch.no_grad():
            p["fb"].clamp_(0.0, 0.95)
            p["depth"].clamp_(0.0, 1.0)
        losses.append(float(loss))
    print("loss", losses[0], losses[-1], {k: v.detach().cpu().numpy() for k, v in p.items()})
    assert losses[-1] / losses[0] < 1e-2
    for k, v in true.items():
        assert float((p[k].detach() - v).abs().max()) < 0.02, k

"""GPU: lightning.LFOExtractionThroughEffect with a sequence of kinds -- the extractor trained through the rendered effects
of a batch that MIXES them (row i is of kind effect[i % len(effect)], the batcher's rule), the mixed twin of
tests/test_gpu_audio_loss_step.py, test_gpu_tremolo_step.py and test_gpu_phaser_step.py.

1. render parity: on a ("flanger", "chorus", "phaser", "tremolo", "dry") batch step.render is the batch's wet, bit for bit, on
   the flanger, chorus, tremolo and dry rows; on the phaser rows it is the render of a single-effect effect="phaser" step on
   those rows gathered into their own batch; the training node's wet_hat has the same bits.
2. gradient decomposition: d loss / d wet_hat once from effect_loss_grad on the full batch; per family, its rows of dry, dy,
   the LFO and the constants gathered into a compact batch and run through the family's un-listed forward and adjoint.  The
   step's h.grad rows are torch.equal to that (one clip per workgroup, a fixed order: nothing depends on the neighbouring
   rows), dry rows are exactly 0.  The fp64 accuracy of each family's adjoint is gated by the per-effect tests; equality
   carries those gates over.  Then one training_step through the Spectral2DCNN reaches every parameter.
3. at the label: without phaser rows every loss of GRAD_NAMES is exactly 0 and the gradient is finite; with phaser rows
   (fixed_lead=0) loss(label) < loss(1 - label) and loss(label) < loss(0.5), strictly, no ratio fixed, values printed.
4. it optimises: the recipe of tests/test_gpu_phaser_step.py::test_it_optimises on ("flanger", "chorus", "phaser"), B = 6;
   the per-kind ratios are printed, not gated.
5. trainer.Trainer drives the module with InterwovenDataModule unchanged.
6. one geometry: effect=("flanger",) gives the loss and gradient bits of effect="flanger"; the same for the tremolo and the
   phaser.
7. a string effect is its un-listed launch sequence, written out by hand: wet_hat, gradient and loss bit for bit."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SR = 44100
FIVE = ("flanger", "chorus", "phaser", "tremolo", "dry")
THREE = ("flanger", "chorus", "phaser")
PHASER_KEYS = ("depth", "centre_frequency_hz", "feedback", "mix")


def batch_of(dev, kinds, B, N, seed, fixed_lead=0):
    from mod_extraction_amd import data_modules
    torch.manual_seed(seed)
    np.random.seed(seed)
    batcher = data_modules.SyntheticFxBatcher(B, N, SR, kinds, dev, audio_seed=seed, fixed_lead=fixed_lead)
    return batcher.render(batcher.sample_params())


def rows_of(kinds, B, *names):
    return [i for i in range(B) if kinds[i % len(kinds)] in names]


def cnn(n):
    from mod_extraction_amd import models
    return models.Spectral2DCNN(in_ch=2, n_samples=n, sr=SR, n_fft=1024, hop_len=256, n_mels=64, kernel_size=(5, 13),
                                out_channels=[64] * 6, temp_dilations=[1, 1, 2, 4, 8, 16], pool_size=(2, 1), latent_dim=1,
                                freq_mask_amount=0.0, time_mask_amount=0.0, use_ln=True)


def test_render_parity(dev):
    from mod_extraction_amd import lightning
    B, N = 10, 22272
    dry, wet, mod, fxp = batch_of(dev, FIVE, B, N, 3, fixed_lead=0)
    assert mod.shape == (B, N // 100)
    step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect=FIVE)
    wet_hat = step.render(dry, mod, fxp)
    assert wet_hat.shape == wet.shape
    same = rows_of(FIVE, B, "flanger", "chorus", "tremolo", "dry")
    ph = rows_of(FIVE, B, "phaser")
    assert same == [0, 1, 3, 4, 5, 6, 8, 9] and ph == [2, 7]
    for kind in ("flanger", "chorus", "tremolo"):                               # the effect did something on these rows
        r = rows_of(FIVE, B, kind)
        assert not torch.equal(wet[r], dry[r]), kind
    assert torch.equal(wet[rows_of(FIVE, B, "dry")], dry[rows_of(FIVE, B, "dry")])
    assert torch.equal(wet_hat[same], wet[same])
    single = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect="phaser")
    want_ph = single.render(dry[ph].contiguous(), mod[ph].contiguous(), {k: fxp[k][ph].contiguous() for k in PHASER_KEYS})
    assert torch.equal(wet_hat[ph], want_ph) and not torch.equal(want_ph, dry[ph])
    h = mod.clone().requires_grad_(True)                                        # the training node renders the same bits
    loss, node_hat = step.audio_loss(h, dry, wet, fxp)
    assert loss.grad_fn is not None and torch.equal(node_hat, wet_hat)


def test_gradient_decomposition(dev):
    from mod_extraction_amd import fx, lightning
    from mod_extraction_amd.effect_losses import effect_loss_grad
    from mod_extraction_amd.util import linear_interpolate_last_dim
    B, N, n_frames = 10, 22272, 88
    weights = {"mrstft": 1.0, "log_mel_l1": 0.5, "l1": 0.5}
    dry, wet, mod, fxp = batch_of(dev, FIVE, B, N, 7, fixed_lead=None)           # the data path's random leads
    torch.manual_seed(1)
    step = lightning.LFOExtractionThroughEffect(cnn(N), sr=SR, effect=FIVE, audio_loss_dict=weights).to(dev).train()
    # an LFO away from the label, at the extractor's rate
    t = torch.linspace(0.0, 1.0, n_frames, device=dev)
    bump = 0.1 * torch.sin(2 * math.pi * (1.5 * t[None, :] + torch.arange(B, device=dev)[:, None] / B))
    h = (linear_interpolate_last_dim(mod, n_frames, align_corners=True) + bump).clamp(0.0, 1.0).clone().requires_grad_(True)
    loss, wet_hat = step.audio_loss(h, dry, wet, fxp)
    loss.backward()
    assert h.grad.shape == (B, n_frames) and torch.isfinite(h.grad).all()
    dy = effect_loss_grad(wet_hat, wet, weights, **step._grad_modules())        # d loss / d wet_hat, once, on the full batch
    assert dy.shape == (B, N) and torch.equal(dy, effect_loss_grad(wet_hat, wet, weights, **step._grad_modules()))
    consts = step.clip_constants(fxp, B, dev)
    m = step._mixed_rows(B, dev)
    x, lfo = dry[:, 0], h.detach()
    for family, names in (("delay", ("flanger", "chorus")), ("tremolo", ("tremolo",)), ("phaser", ("phaser",))):
        r = rows_of(FIVE, B, *names)
        assert r == m[family].tolist() and len(r) >= 2
        xc, dyc, hc = x[r].contiguous(), dy[r].contiguous(), lfo[r].contiguous()
        cc = {k: v[r].contiguous() for k, v in consts.items()}
        if family == "delay":
            md, M = m["max_delay"][r].contiguous(), m["max_delay_max"]
            assert sorted(set(md.tolist())) == [485, 1764]                       # both geometries in one launch
            y, st = fx.flanger_forward_stash(xc, hc, cc, md, M)
            want = fx.flanger_backward(dyc, xc, hc, st, cc, md, M, need_dx=False, params=())[1]
        elif family == "tremolo":
            y = fx.tremolo_forward(xc, hc, cc)
            want = fx.tremolo_backward(dyc, xc, hc, cc, need_dx=False, need_dmix=False)[1]
        else:
            y, st, _ = fx.phaser_forward_stash_lr(xc, cc, None, SR, N, hc)
            want = fx.phaser_backward_lr(dyc, xc, st, cc, None, SR, N, n_frames, need_dx=False, params_wanted=())[1]
        assert torch.equal(wet_hat[r, 0], y), family
        assert float(want.abs().max()) > 0 and torch.isfinite(want).all(), family
        differ = int((h.grad[r] != want).sum())
        print(f"{family}: rows {r}, max |grad| {float(want.abs().max()):.3e}, {differ} of {want.numel()} values differ")
        assert torch.equal(h.grad[r], want), family
    r = rows_of(FIVE, B, "dry")
    assert len(r) == 2 and (h.grad[r] == 0).all() and torch.equal(wet_hat[r], dry[r])
    # through the extractor: one training step's backward reaches every parameter
    step.zero_grad()
    loss = step.training_step((dry, wet, None, fxp))
    assert loss.grad_fn is not None and math.isfinite(float(loss)) and float(loss) > 0
    loss.backward()
    for name, p in step.model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().sum()) > 0, name
    assert math.isfinite(float(step.logged["train/loss"][-1]))


def test_zero_at_the_label_without_phaser_rows(dev):
    from mod_extraction_amd import lightning
    from mod_extraction_amd.effect_losses import GRAD_NAMES
    kinds = ("flanger", "chorus", "tremolo", "dry")
    B, N = 8, 22272
    dry, wet, mod, fxp = batch_of(dev, kinds, B, N, 5)
    step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect=kinds,
                                                audio_loss_dict={k: 1.0 for k in GRAD_NAMES})
    assert torch.equal(step.render(dry, mod, fxp), wet) and float(wet.abs().max()) > 0.1
    h = mod.clone().requires_grad_(True)
    loss, wet_hat = step.audio_loss(h, dry, wet, fxp, prefix="train")
    assert loss.grad_fn is not None and torch.equal(wet_hat, wet) and float(loss) == 0.0
    for k in GRAD_NAMES:
        assert float(step.logged[f"train/{k}"][-1]) == 0.0, k
    loss.backward()
    assert h.grad.shape == mod.shape
    for k in GRAD_NAMES:                                                        # each loss alone: which one, if any, is not finite
        one = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect=kinds, audio_loss_dict={k: 1.0})
        hk = mod.clone().requires_grad_(True)
        lk, _ = one.audio_loss(hk, dry, wet, fxp)
        lk.backward()
        print(f"{k}: loss at the label {float(lk)}, gradient finite {bool(torch.isfinite(hk.grad).all())}, "
              f"max |grad| {float(hk.grad.abs().nan_to_num(posinf=float('inf')).max()):.3e}")
        assert float(lk) == 0.0 and torch.isfinite(hk.grad).all(), k
    assert torch.isfinite(h.grad).all()


@pytest.mark.parametrize("name", ["mrstft", "log_mel_l1"])
def test_near_the_label_with_phaser_rows(dev, name):
    from mod_extraction_amd import lightning
    B, N = 6, 88200
    dry, wet, mod, fxp = batch_of(dev, THREE, B, N, 5, fixed_lead=0)
    assert int(fxp["lead"].max()) == 0
    step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect=THREE, audio_loss_dict={name: 1.0})
    with torch.no_grad():
        at_label = float(step.audio_loss(mod, dry, wet, fxp)[0])
        at_mirror = float(step.audio_loss((1.0 - mod).contiguous(), dry, wet, fxp)[0])
        at_half = float(step.audio_loss(torch.full_like(mod, 0.5), dry, wet, fxp)[0])
    print(f"{name}: loss(label) {at_label:.6e}, loss(1 - label) {at_mirror:.6e}, loss(0.5) {at_half:.6e}")
    assert math.isfinite(at_label) and at_label < at_mirror
    assert at_label < at_half


@pytest.mark.parametrize("name", ["mrstft", "log_mel_l1"])
def test_it_optimises(dev, name):
    from mod_extraction_amd import lightning
    from mod_extraction_amd.util import linear_interpolate_last_dim
    B, N, n_frames = 6, 88200, 345
    dry, wet, mod, fxp = batch_of(dev, THREE, B, N, 11, fixed_lead=0)
    step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect=THREE, audio_loss_dict={name: 1.0})
    label = linear_interpolate_last_dim(mod, n_frames, align_corners=True)
    t = torch.linspace(0.0, 1.0, n_frames, device=dev)
    bump = 0.05 * torch.sin(2 * math.pi * (1.5 * t[None, :] + torch.arange(B, device=dev)[:, None] / B))
    h = (label + bump).clamp(0.0, 1.0).clone().requires_grad_(True)
    opt = torch.optim.Adam([h], lr=1e-3)
    start = (h.detach() - label).abs().mean(1)
    dist0 = float(start.mean())
    losses = []
    for _ in range(80):
        opt.zero_grad()
        loss, _ = step.audio_loss(h, dry, wet, fxp)
        loss.backward()
        opt.step()
        with torch.no_grad():
            h.clamp_(0.0, 1.0)
        losses.append(float(loss))
    with torch.no_grad():
        final = float(step.audio_loss(h.detach(), dry, wet, fxp)[0])
    end = (h.detach() - label).abs().mean(1)
    dist1 = float(end.mean())
    print(name, "loss", losses[0], "->", final, "ratio", final / losses[0], "| L1 to the label", dist0, "->", dist1,
          "ratio", dist1 / dist0)
    for kind in THREE:                                                          # information, not gated
        r = rows_of(THREE, B, kind)
        print(f"  {kind}: L1 to the label {float(start[r].mean()):.6e} -> {float(end[r].mean()):.6e}, "
              f"ratio {float(end[r].mean() / start[r].mean()):.4f}")
    assert final < losses[0]
    assert dist1 < dist0


def test_trainer_integration(dev):
    from mod_extraction_amd import data_modules, lightning, optim, trainer
    N = 22272
    torch.manual_seed(2)
    np.random.seed(2)
    step = lightning.LFOExtractionThroughEffect(cnn(N), sr=SR, effect=THREE,
                                                audio_loss_dict={"mrstft": 1.0, "esr": 0.0}).to(dev).train()
    opt = optim.FlatAdamW(step.parameters(), lr=1e-4, betas=(0.8, 0.99))
    dm = data_modules.InterwovenDataModule(batch_size=6, shared_args={"n_samples": N, "sr": SR},
                                           shared_train_args={"num_examples_per_epoch": 12},
                                           shared_val_args={"num_examples_per_epoch": 6}, overlap=False)
    assert tuple(dm.kinds) == step.kinds
    dm.setup(dev, rank=0, seed=9)
    before = [p.detach().clone() for p in step.parameters()]
    seen = []
    keep = step.log
    step.log = lambda n, v: (seen.append((n, float(v))), keep(n, v))[1]
    hist = trainer.Trainer(max_epochs=2, log_fn=None).fit(step, dm, opt)
    train_losses = [v for n, v in seen if n == "train/loss"]
    assert len(train_losses) == 4 and all(math.isfinite(v) for v in train_losses)
    assert len(hist) == 2
    for k in ("train/loss", "train/mrstft", "train/esr", "val/loss", "val/mrstft"):
        assert math.isfinite(hist[-1][k]), k
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, step.parameters()))


def test_one_geometry_is_the_single_effect_step(dev):
    from mod_extraction_amd import lightning
    B, N = 4, 22272
    weights = {"mrstft": 1.0, "log_mel_l1": 0.5, "l1": 0.5}
    for effect in ("flanger", "tremolo", "phaser"):
        dry, wet, mod, fxp = batch_of(dev, (effect,), B, N, 13, fixed_lead=0)
        h0 = (0.9 * mod + 0.05).contiguous()
        out = []
        for e in (effect, (effect,)):
            step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect=e, audio_loss_dict=weights)
            h = h0.clone().requires_grad_(True)
            loss, wet_hat = step.audio_loss(h, dry, wet, fxp)
            loss.backward()
            out.append((loss.detach(), wet_hat, h.grad))
            if effect != "phaser":                                              # the phaser's lead-in rule: near, not equal
                assert torch.equal(step.render(dry, mod, fxp), wet), effect
        (l0, w0, g0), (l1, w1, g1) = out
        assert float(l0) > 0 and float(g0.abs().max()) > 0, effect
        assert torch.equal(l0, l1) and torch.equal(w0, w1) and torch.equal(g0, g1), effect


@pytest.mark.parametrize("effect", ["flanger", "tremolo", "phaser"])
def test_string_effect_is_its_unlisted_launch_sequence(dev, effect):
    """effect="flanger" / "tremolo" / "phaser" against the launch sequence written out by hand, no step code: the
    ``fx.derive_*`` constants, the family's un-listed stash forward, ``effect_loss_grad``, the un-listed adjoint asked for
    dmod alone, the weighted sum in dict order.  wet_hat, the gradient and the loss are torch.equal to those."""
    from mod_extraction_amd import fx, lightning
    from mod_extraction_amd.effect_losses import effect_loss_grad, effect_loss_terms
    from mod_extraction_amd.util import linear_interpolate_last_dim
    B, N, n_frames = 3, 22272, 88
    weights = {"mrstft": 1.0, "log_mel_l1": 0.5, "l1": 0.5}
    dry, wet, mod, fxp = batch_of(dev, (effect,), B, N, 17, fixed_lead=0)
    step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect=effect, audio_loss_dict=weights)
    t = torch.linspace(0.0, 1.0, n_frames, device=dev)                          # an LFO away from the label
    bump = 0.1 * torch.sin(2 * math.pi * (1.5 * t[None, :] + torch.arange(B, device=dev)[:, None] / B))
    h = (linear_interpolate_last_dim(mod, n_frames, align_corners=True) + bump).clamp(0.0, 1.0).clone().requires_grad_(True)
    loss, wet_hat = step.audio_loss(h, dry, wet, fxp)
    loss.backward()
    x, lfo = dry[:, 0], h.detach()
    if effect == "flanger":
        c = fx.derive_clip_constants(B, dev, 44, 441, fxp["feedback"], fxp["min_delay_width"], fxp["width"], fxp["depth"],
                                     fxp["mix"], check=False)
        md = torch.full((B,), 485, device=dev, dtype=torch.int32)
        y, st = fx.flanger_forward_stash(x, lfo, c, md, 485)
    elif effect == "tremolo":
        c = fx.derive_tremolo_constants(B, dev, fxp["mix"], check=False)
        y = fx.tremolo_forward(x, lfo, c)
    else:
        c = fx.derive_phaser_params(B, dev, fxp["depth"], fxp["centre_frequency_hz"], fxp["feedback"], fxp["mix"], check=False)
        y, st, _ = fx.phaser_forward_stash_lr(x, c, None, SR, N, lfo)
    weighted = {}
    dy = effect_loss_grad(y.unsqueeze(1), wet, weights, values=weighted, **step._grad_modules())
    if effect == "flanger":
        want = fx.flanger_backward(dy, x, lfo, st, c, md, 485, need_dx=False, params=())[1]
    elif effect == "tremolo":
        want = fx.tremolo_backward(dy, x, lfo, c, need_dx=False, need_dmix=False)[1]
    else:
        want = fx.phaser_backward_lr(dy, x, st, c, None, SR, N, n_frames, need_dx=False, params_wanted=())[1]
    terms = {k: v / weights[k] for k, v in weighted.items()}
    terms["l1"] = effect_loss_terms(y.unsqueeze(1), wet)["l1"]
    want_loss = 1.0 * terms["mrstft"] + 0.5 * terms["log_mel_l1"] + 0.5 * terms["l1"]
    print(f"{effect}: loss {float(loss.detach()):.6e} (by hand {float(want_loss):.6e}), max |grad| {float(want.abs().max()):.3e}, "
          f"{int((h.grad != want).sum())} of {want.numel()} gradient values and "
          f"{int((wet_hat[:, 0] != y).sum())} of {y.numel()} samples differ")
    assert not torch.equal(y, x) and float(want.abs().max()) > 0 and torch.isfinite(want).all()
    assert torch.equal(wet_hat[:, 0], y)
    assert h.grad.shape == (B, n_frames) and torch.equal(h.grad, want)
    assert float(loss) > 0 and torch.equal(loss.detach(), want_loss)

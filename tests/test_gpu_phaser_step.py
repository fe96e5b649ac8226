"""GPU: lightning.LFOExtractionThroughEffect(effect="phaser") on ("phaser",) batches of the device data path -- the phaser
twin of tests/test_gpu_audio_loss_step.py and tests/test_gpu_tremolo_step.py.

1. render parity: step.render (expand + stash forward, lead 0) equals fx.PhaserModule.forward on the expanded row, bit for
   bit, and so does the wet_hat of the training node.
2. near the truth: the step re-renders from dry alone with lead 0 and empty filter state, while the batch's wet came from
   JUCE's oscillator (class docstring: start transient, cut-off grid, a linearly interpolated label), so the loss at the
   label is small but not 0.  Asserted, for mrstft and for log_mel_l1, with fixed_lead=0: loss(label) < loss(1 - label) and
   loss(label) < loss(constant 0.5), strictly, no ratio fixed; the three values are printed.
3. chain gradient: the step's d loss / d mod_sig_hat against effect_loss_grad on wet_hat followed by the fp64 phaser adjoint
   (tests/helpers/phaser_adjoint64.py, at the stash forward's own clip decisions and osc row) and the fp64 gather
   (tests/helpers/phaser_lr64.py); gate GATES["dmod_lo"] of tests/test_gpu_phaser_grad.py (the batcher draws feedback <=
   0.7).  Then one training_step through the Spectral2DCNN reaches every parameter.
4. it optimises: Adam on a free (B, 345) LFO from the label plus a smooth bump lowers the loss and the L1 distance to the
   label (gated as "decreases" only; both ratios are printed).
5. trainer.Trainer drives the module with the phaser data module unchanged: two epochs of two steps."""
import math

import numpy as np
import pytest
import torch

from tests.helpers import phaser_adjoint64 as pa
from tests.helpers.phaser_lr64 import gather64
from tests.test_gpu_phaser_grad import GATES, gpu_decisions, normwise

pytestmark = pytest.mark.gpu
SR = 44100


def batch_of(dev, B, N, seed, fixed_lead=0):
    from mod_extraction_amd import data_modules
    torch.manual_seed(seed)
    np.random.seed(seed)
    batcher = data_modules.SyntheticFxBatcher(B, N, SR, ("phaser",), dev, audio_seed=seed, fixed_lead=fixed_lead)
    return batcher.render(batcher.sample_params())


def cnn(n):
    from mod_extraction_amd import models
    return models.Spectral2DCNN(in_ch=2, n_samples=n, sr=SR, n_fft=1024, hop_len=256, n_mels=64, kernel_size=(5, 13),
                                out_channels=[64] * 6, temp_dilations=[1, 1, 2, 4, 8, 16], pool_size=(2, 1), latent_dim=1,
                                freq_mask_amount=0.0, time_mask_amount=0.0, use_ln=True)


def test_render_parity(dev):
    from mod_extraction_amd import fx, lightning
    B, N = 4, 22272
    dry, wet, mod, fxp = batch_of(dev, B, N, 3)
    assert mod.shape == (B, N // 100) and float(wet.abs().max()) > 0.1 and not torch.equal(wet, dry)
    step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect="phaser")
    wet_hat = step.render(dry, mod, fxp)
    assert wet_hat.shape == wet.shape
    mod_g = fx.phaser_mod_expand(mod.contiguous(), None, N, N)
    want = fx.PhaserModule(SR)(dry, mod_sig=mod_g, depth=fxp["depth"], centre_frequency_hz=fxp["centre_frequency_hz"],
                               feedback=fxp["feedback"], mix=fxp["mix"])
    assert torch.equal(wet_hat, want)
    # fx_params needs only the four parameters: rate_hz and lead are ignored
    four = {k: fxp[k] for k in ("depth", "centre_frequency_hz", "feedback", "mix")}
    assert torch.equal(step.render(dry, mod, four), want)
    h = mod.clone().requires_grad_(True)                                       # the training node renders the same bits
    loss, wet_hat = step.audio_loss(h, dry, wet, four)
    assert loss.grad_fn is not None and torch.equal(wet_hat, want)


@pytest.mark.parametrize("name", ["mrstft", "log_mel_l1"])
def test_near_the_truth(dev, name):
    from mod_extraction_amd import lightning
    B, N = 6, 88200
    dry, wet, mod, fxp = batch_of(dev, B, N, 5, fixed_lead=0)
    assert int(fxp["lead"].max()) == 0
    step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect="phaser", audio_loss_dict={name: 1.0})
    with torch.no_grad():
        at_label = float(step.audio_loss(mod, dry, wet, fxp)[0])
        at_mirror = float(step.audio_loss((1.0 - mod).contiguous(), dry, wet, fxp)[0])
        at_half = float(step.audio_loss(torch.full_like(mod, 0.5), dry, wet, fxp)[0])
    print(f"{name}: loss(label) {at_label:.6e}, loss(1 - label) {at_mirror:.6e}, loss(0.5) {at_half:.6e}")
    assert math.isfinite(at_label) and at_label < at_mirror
    assert at_label < at_half


def test_chain_gradient(dev):
    from mod_extraction_amd import fx, lightning
    from mod_extraction_amd.effect_losses import effect_loss_grad
    B, N = 4, 22272
    weights = {"mrstft": 1.0, "log_mel_l1": 0.5, "l1": 0.5}
    dry, wet, mod, fxp = batch_of(dev, B, N, 7, fixed_lead=None)               # the data path's random leads
    assert float(fxp["feedback"].abs().max()) <= 0.7
    torch.manual_seed(1)
    step = lightning.LFOExtractionThroughEffect(cnn(N), sr=SR, effect="phaser", audio_loss_dict=weights).to(dev).train()
    hat, _ = step.model(lightning.stack_dry_wet(dry, wet))
    h = hat.detach().squeeze(1).clone().requires_grad_(True)
    assert h.shape == (B, 88)
    loss, wet_hat = step.audio_loss(h, dry, wet, fxp)
    loss.backward()
    assert h.grad.shape == h.shape and torch.isfinite(h.grad).all()
    # the composition: d loss / d wet_hat from the loss kernels, the fp64 adjoint at group rate, the fp64 gather
    dy = effect_loss_grad(wet_hat, wet, weights)
    consts = step.clip_constants(fxp, B, dev)
    y, st, mod_g = fx.phaser_forward_stash_lr(dry[:, 0], consts, None, SR, N, h.detach().contiguous())   # the node's launches
    assert torch.equal(y, wet_hat[:, 0])
    osc = (np.float32(1.0) - np.float32(2.0) * mod_g.cpu().numpy()).astype(np.float32)
    params = {k: v.cpu().numpy() for k, v in consts.items()}
    x_np, dy_np = dry[:, 0].cpu().numpy(), dy.cpu().numpy()
    ref = pa.phaser_adjoint64(x_np, osc, params, float(SR), dy_np)
    mine = gpu_decisions(st, N, N)
    flips = int((mine != ref["pass_m"]).sum())
    print(f"chain: {flips} output-clip decisions differ between the scan forward and the sequential fp32 forward")
    if flips:
        ref = pa.phaser_adjoint64(x_np, osc, params, float(SR), dy_np, fwd32=ref["fwd32"], pass_m=mine)
    want = gather64(ref["dmod"], [0] * B, N, h.size(1))
    err = normwise(h.grad.cpu().numpy(), want)
    print(f"chain gradient error {err:.3e} (gate {GATES['dmod_lo']:.1e}), loss {float(loss):.6e}")
    assert err < GATES["dmod_lo"]
    # through the extractor: one training step's backward reaches every parameter
    step.zero_grad()
    loss = step.training_step((dry, wet, None, fxp))
    assert loss.grad_fn is not None and math.isfinite(float(loss)) and float(loss) > 0
    loss.backward()
    for name, p in step.model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().sum()) > 0, name
    assert math.isfinite(float(step.logged["train/loss"][-1]))


@pytest.mark.parametrize("name", ["mrstft", "log_mel_l1"])
def test_it_optimises(dev, name):
    from mod_extraction_amd import lightning
    from mod_extraction_amd.util import linear_interpolate_last_dim
    B, N, n_frames = 4, 88200, 345
    dry, wet, mod, fxp = batch_of(dev, B, N, 11, fixed_lead=0)
    step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect="phaser", audio_loss_dict={name: 1.0})
    label = linear_interpolate_last_dim(mod, n_frames, align_corners=True)
    t = torch.linspace(0.0, 1.0, n_frames, device=dev)
    bump = 0.05 * torch.sin(2 * math.pi * (1.5 * t[None, :] + torch.arange(B, device=dev)[:, None] / B))
    h = (label + bump).clamp(0.0, 1.0).clone().requires_grad_(True)
    opt = torch.optim.Adam([h], lr=1e-3)
    dist0 = float((h.detach() - label).abs().mean())
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
    dist1 = float((h.detach() - label).abs().mean())
    print(name, "loss", losses[0], "->", final, "ratio", final / losses[0], "| L1 to the label", dist0, "->", dist1,
          "ratio", dist1 / dist0)
    assert final < losses[0]
    assert dist1 < dist0


def test_trainer_integration(dev):
    from mod_extraction_amd import data_modules, lightning, optim, trainer
    N = 22272
    torch.manual_seed(2)
    np.random.seed(2)
    step = lightning.LFOExtractionThroughEffect(cnn(N), sr=SR, effect="phaser",
                                                audio_loss_dict={"mrstft": 1.0, "esr": 0.0}).to(dev).train()
    opt = optim.FlatAdamW(step.parameters(), lr=1e-4, betas=(0.8, 0.99))
    dm = data_modules.PedalboardPhaserDataModule(batch_size=4, n_samples=N, sr=SR, train_num_examples_per_epoch=8,
                                                 val_num_examples_per_epoch=4, overlap=False)
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

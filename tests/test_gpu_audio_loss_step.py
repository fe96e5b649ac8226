"""GPU: lightning.LFOExtractionThroughEffect -- the extractor trained through the rendered flanger with an audio loss.

1. zero at the truth: a re-render of the batch's dry clips from the batch's own 882-point LFO and fx_params is the batch's
   wet, bit for bit, through both the no-grad render and the training node, and every loss of GRAD_NAMES is exactly 0.0;
2. chain gradient: the step's d loss / d mod_sig_hat against the composition of the separately tested pieces --
   effect_loss_grad on wet_hat (tests/test_gpu_mrstft*.py, test_gpu_logmel_loss.py), then the fp64 low-rate adjoint
   (tests/helpers/flanger_adjoint64_lr.py).  The loss gradient fed to the fp64 adjoint is the kernels' own output, so the
   only error under test is the adjoint's: gate 3e-6 norm-wise, the dmod gate of tests/test_gpu_flanger_lowrate_grad.py
   (feedback <= 0.7, the data path's range), without widening;
3. it optimises: Adam on a free (B, 345) LFO from the truth plus a smooth perturbation lowers the loss and the L1 distance
   to the unperturbed LFO (gated as "decreases" only; both ratios are printed);
4. trainer.Trainer drives the module unchanged."""
import math

import numpy as np
import pytest
import torch

from tests.helpers.flanger_adjoint64_lr import flanger_adjoint64_lr
from tests.test_gpu_flanger_grad import normwise

pytestmark = pytest.mark.gpu
SR = 44100


def batch_of(dev, B, N, seed):
    from mod_extraction_amd import data_modules
    torch.manual_seed(seed)
    np.random.seed(seed)
    batcher = data_modules.SyntheticFxBatcher(B, N, SR, ("flanger",), dev, audio_seed=seed)
    return batcher.render(batcher.sample_params())


def cnn(n):
    from mod_extraction_amd import models
    return models.Spectral2DCNN(in_ch=2, n_samples=n, sr=SR, n_fft=1024, hop_len=256, n_mels=64, kernel_size=(5, 13),
                                out_channels=[64] * 6, temp_dilations=[1, 1, 2, 4, 8, 16], pool_size=(2, 1), latent_dim=1,
                                freq_mask_amount=0.0, time_mask_amount=0.0, use_ln=True)


def test_zero_at_the_truth(dev):
    from mod_extraction_amd import lightning
    from mod_extraction_amd.effect_losses import GRAD_NAMES
    B, N = 6, 88200
    dry, wet, mod, fxp = batch_of(dev, B, N, 3)
    assert mod.shape == (B, 882)
    step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, audio_loss_dict={k: 1.0 for k in GRAD_NAMES})
    wet_hat = step.render(dry, mod, fxp)
    assert torch.equal(wet_hat, wet) and float(wet.abs().max()) > 0.1
    loss, wet_hat, = step.audio_loss(mod, dry, wet, fxp, prefix="val")
    assert torch.equal(wet_hat, wet) and float(loss) == 0.0
    for k in GRAD_NAMES:
        assert float(step.logged[f"val/{k}"][-1]) == 0.0, k
    step.logged.clear()
    h = mod.clone().requires_grad_(True)                                       # the training node: stash forward + losses
    loss, wet_hat = step.audio_loss(h, dry, wet, fxp, prefix="train")
    assert loss.grad_fn is not None and torch.equal(wet_hat, wet) and float(loss) == 0.0
    for k in GRAD_NAMES:
        assert float(step.logged[f"train/{k}"][-1]) == 0.0, k
    loss.backward()
    assert h.grad.shape == mod.shape                 # (its value at the exact minimum is the losses' own 0 / 0 convention)
    print("gradient at the truth finite:", bool(torch.isfinite(h.grad).all()))


@pytest.mark.parametrize("weights", [{"mrstft": 1.0}, {"log_mel_l1": 1.0, "l1": 0.5, "esr": 0.25}])
def test_chain_gradient(dev, weights):
    from mod_extraction_amd import lightning
    from mod_extraction_amd.effect_losses import effect_loss_grad
    B, N = 4, 22272
    dry, wet, mod, fxp = batch_of(dev, B, N, 5)
    torch.manual_seed(1)
    step = lightning.LFOExtractionThroughEffect(cnn(N), sr=SR, audio_loss_dict=weights).to(dev).train()
    hat, _ = step.model(lightning.stack_dry_wet(dry, wet))
    h = hat.detach().squeeze(1).clone().requires_grad_(True)
    assert h.shape == (B, 88)
    loss, wet_hat = step.audio_loss(h, dry, wet, fxp)
    loss.backward()
    # the composition: d loss / d wet_hat from the loss kernels, then the fp64 adjoint at the low rate
    dy = effect_loss_grad(wet_hat, wet, weights)
    consts = {k: v.cpu().numpy() for k, v in step.clip_constants(fxp, B, dev).items()}
    ref = flanger_adjoint64_lr(dry[:, 0].cpu().numpy(), h.detach().cpu().numpy(), consts, step.max_delay_samples, dy.cpu().numpy())
    assert np.array_equal(ref["fwd"]["y32"], wet_hat[:, 0].cpu().numpy())
    err = normwise(h.grad.cpu().numpy(), ref["dmod"], slice(None))
    print(weights, "chain gradient error", err, "loss", float(loss))
    assert err < 3e-6
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
    dry, wet, mod, fxp = batch_of(dev, B, N, 11)
    step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, audio_loss_dict={name: 1.0})
    truth = linear_interpolate_last_dim(mod, n_frames, align_corners=True)
    t = torch.linspace(0.0, 1.0, n_frames, device=dev)
    bump = 0.05 * torch.sin(2 * math.pi * (1.5 * t[None, :] + torch.arange(B, device=dev)[:, None] / B))
    h = (truth + bump).clamp(0.0, 1.0).clone().requires_grad_(True)
    opt = torch.optim.Adam([h], lr=1e-3)
    dist0 = float((h.detach() - truth).abs().mean())
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
    dist1 = float((h.detach() - truth).abs().mean())
    print(name, "loss", losses[0], "->", final, "ratio", final / losses[0], "| L1 to the truth", dist0, "->", dist1,
          "ratio", dist1 / dist0)
    assert final < losses[0]
    assert dist1 < dist0


def test_trainer_integration(dev):
    from mod_extraction_amd import data_modules, lightning, optim, trainer
    N = 22272
    torch.manual_seed(2)
    np.random.seed(2)
    step = lightning.LFOExtractionThroughEffect(cnn(N), sr=SR, audio_loss_dict={"mrstft": 1.0, "esr": 0.0},
                                                loss_dict={"l1": 0.1}).to(dev).train()
    opt = optim.FlatAdamW(step.parameters(), lr=1e-4, betas=(0.8, 0.99))
    dm = data_modules.FlangerCPUDataModule(batch_size=4, n_samples=N, sr=SR, train_num_examples_per_epoch=12,
                                           val_num_examples_per_epoch=4, overlap=False)
    dm.setup(dev, rank=0, seed=9)
    before = [p.detach().clone() for p in step.parameters()]
    seen = []
    keep = step.log
    step.log = lambda n, v: (seen.append((n, float(v))), keep(n, v))[1]
    hist = trainer.Trainer(max_epochs=1, log_fn=None).fit(step, dm, opt)
    train_losses = [v for n, v in seen if n == "train/loss"]
    assert len(train_losses) == 3 and all(math.isfinite(v) for v in train_losses)
    for k in ("train/loss", "train/mrstft", "train/esr", "train/lfo_l1", "val/loss", "val/mrstft"):
        assert math.isfinite(hist[0][k]), k
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, step.parameters()))
    step.eval()
    loss, data, _ = step.validation_step(dm.val_batch())
    assert loss.grad_fn is None and not loss.requires_grad
    assert data["wet_hat"].shape == data["wet"].shape and not data["wet_hat"].requires_grad
    assert torch.isfinite(data["wet_hat"]).all()


def test_smoothing_crops_dry_and_wet(dev):
    """model_smooth_n_frames > 1: the LFO loses frames, dry and wet are centre-cropped by the TBPTT rule, and the step still
    trains (the first max_delay samples of wet_hat differ from wet by construction: documented in the class)."""
    from mod_extraction_amd import lightning
    B, N = 4, 22272
    dry, wet, mod, fxp = batch_of(dev, B, N, 13)
    torch.manual_seed(4)
    step = lightning.LFOExtractionThroughEffect(cnn(N), sr=SR, model_smooth_n_frames=4,
                                                audio_loss_dict={"l1": 1.0, "mrstft": 0.5}).to(dev).train()
    loss, data, _ = step.common_step((dry, wet, mod, fxp), is_training=True)
    n_f = data["mod_sig_hat"].size(-1)
    assert n_f < 88 and data["wet_hat"].size(-1) == int(n_f / 88 * N) == data["wet"].size(-1) == data["dry"].size(-1)
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in step.model.parameters())

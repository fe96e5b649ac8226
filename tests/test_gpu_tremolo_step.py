"""GPU: lightning.LFOExtractionThroughEffect(effect="tremolo") on ("tremolo",) batches of the device data path -- the
tremolo twin of tests/test_gpu_audio_loss_step.py.

1. zero at the truth: the batch's wet is fx.py:13-22 on the batch's dry and resampled label (checked against the torch
   expression on the host, which tests/test_param_stream.py pins to the reference), the re-render from the batch's own
   882-point LFO and mix is that wet bit for bit through both the no-grad render and the training node, and every loss of
   GRAD_NAMES is exactly 0.0;
2. chain gradient: the step's d loss / d mod_sig_hat against effect_loss_grad on wet_hat followed by the fp64 adjoint
   (tests/helpers/tremolo_adjoint64.py), gate 3e-6 norm-wise (the dmod gate of the flanger step); then one training_step
   through the Spectral2DCNN reaches every parameter;
3. it optimises: Adam on a free (B, 345) LFO from the truth plus a smooth perturbation lowers the loss and the L1 distance
   to the truth (gated as "decreases" only; both ratios are printed);
4. an interwoven ("flanger", "tremolo", "dry") batch: every row group equals the render of a single-kind batcher given the
   same audio seed and parameters."""
import math

import numpy as np
import pytest
import torch

from tests.helpers.tremolo_adjoint64 import tremolo_adjoint64
from tests.test_gpu_flanger_grad import normwise

pytestmark = pytest.mark.gpu
SR = 44100


def batcher_of(dev, B, N, seed, kinds=("tremolo",)):
    from mod_extraction_amd import data_modules
    torch.manual_seed(seed)
    np.random.seed(seed)
    return data_modules.SyntheticFxBatcher(B, N, SR, kinds, dev, audio_seed=seed)


def batch_of(dev, B, N, seed):
    batcher = batcher_of(dev, B, N, seed)
    return batcher.render(batcher.sample_params())


def cnn(n):
    from mod_extraction_amd import models
    return models.Spectral2DCNN(in_ch=2, n_samples=n, sr=SR, n_fft=1024, hop_len=256, n_mels=64, kernel_size=(5, 13),
                                out_channels=[64] * 6, temp_dilations=[1, 1, 2, 4, 8, 16], pool_size=(2, 1), latent_dim=1,
                                freq_mask_amount=0.0, time_mask_amount=0.0, use_ln=True)


def test_zero_at_the_truth(dev):
    from mod_extraction_amd import fx, lightning
    from mod_extraction_amd.effect_losses import GRAD_NAMES
    from mod_extraction_amd.util import linear_interpolate_last_dim
    B, N = 6, 88200
    dry, wet, mod, fxp = batch_of(dev, B, N, 3)
    assert mod.shape == (B, 882) and float(wet.abs().max()) > 0.1 and not torch.equal(wet, dry)
    # the data path is the reference's expression: fx.py:13-22 on the host, one clip at a time (its mix is a scalar)
    up = linear_interpolate_last_dim(mod, N, align_corners=True).cpu()
    for b in range(B):
        want = fx.apply_tremolo(dry[b:b + 1].cpu(), up[b:b + 1], float(fxp["mix"][b]))
        assert torch.equal(wet[b:b + 1].cpu(), want), b
    step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect="tremolo",
                                                audio_loss_dict={k: 1.0 for k in GRAD_NAMES})
    wet_hat = step.render(dry, mod, {"mix": fxp["mix"]})                        # fx_params needs only mix
    assert torch.equal(wet_hat, wet)
    loss, wet_hat, = step.audio_loss(mod, dry, wet, fxp, prefix="val")
    assert torch.equal(wet_hat, wet) and float(loss) == 0.0
    for k in GRAD_NAMES:
        assert float(step.logged[f"val/{k}"][-1]) == 0.0, k
    step.logged.clear()
    h = mod.clone().requires_grad_(True)                                       # the training node
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
    step = lightning.LFOExtractionThroughEffect(cnn(N), sr=SR, effect="tremolo", audio_loss_dict=weights).to(dev).train()
    hat, _ = step.model(lightning.stack_dry_wet(dry, wet))
    h = hat.detach().squeeze(1).clone().requires_grad_(True)
    assert h.shape == (B, 88)
    loss, wet_hat = step.audio_loss(h, dry, wet, fxp)
    loss.backward()
    # the composition: d loss / d wet_hat from the loss kernels, then the fp64 adjoint at the low rate
    dy = effect_loss_grad(wet_hat, wet, weights)
    consts = {k: v.cpu().numpy() for k, v in step.clip_constants(fxp, B, dev).items()}
    ref = tremolo_adjoint64(dry[:, 0].cpu().numpy(), h.detach().cpu().numpy(), consts["mix"], dy.cpu().numpy(),
                            omm=consts["one_minus_mix"])
    assert float(np.abs(ref["y"] - wet_hat[:, 0].cpu().numpy()).max()) < 1e-6
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
    step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect="tremolo", audio_loss_dict={name: 1.0})
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


def test_interwoven_batch(dev):
    B, N, seed = 6, 22272, 21
    mixed = batcher_of(dev, B, N, seed, ("flanger", "tremolo", "dry"))
    p = mixed.sample_params()
    dry, wet, mod, fxp = mixed.render(p)
    assert mixed.kinds == ["flanger", "tremolo", "dry"] * 2
    assert float(fxp["mix"][1]) == float(p["mix"][1]) and 0.0 <= float(p["mix"][1]) <= 1.0
    for kind, rows in (("flanger", [0, 3]), ("tremolo", [1, 4]), ("dry", [2, 5])):
        single = batcher_of(dev, B, N, seed, (kind,))
        d1, w1, m1, _ = single.render(p)                      # the same parameters and noise, every row of one kind
        assert torch.equal(d1, dry) and torch.equal(m1, mod), kind
        assert torch.equal(w1[rows], wet[rows]), kind
        others = [r for r in range(B) if r not in rows]
        assert not torch.equal(w1[others], wet[others]), kind
    assert torch.equal(wet[[2, 5]], dry[[2, 5]]) and not torch.equal(wet[[1, 4]], dry[[1, 4]])

"""Set-up and torchrun worker of tests/test_gpu_trainer_clip_accum.py: the module, clips and seeds of
ddp_equivalence_worker.py (mode "lfo": 4 clips of 22 272 samples; mode "tbptt": 4 chunks of 1024 samples) driven through
`trainer.Trainer.fit` with the gradient-clipping / accumulation keys.  The extractor's mask amounts are 0, so the `train()` that
`fit` switches on draws no mask: the step is the `.eval()` step of the original worker.

As a script (launched by torch.distributed.run with WORLD_SIZE ranks sharing one GPU, MODEX_SHARE_GPU=1, gloo):
    clip_accum_worker.py OUT TOTAL CLIP_VAL
every rank takes its slice of the fixed batch, runs ONE optimizer step through `Trainer(gradient_clip_val=CLIP_VAL).fit` and
saves OUT.rank<r> = {param, grad (averaged), norm, scale}."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from mod_extraction_amd import lightning, models, optim, trainer  # noqa: E402


class ListData:
    """The data-module surface `Trainer.fit` needs, over a fixed list of training batches (no validation)."""

    def __init__(self, batches):
        self.batches, self.i = list(batches), 0

    def train_steps_per_epoch(self):
        return len(self.batches)

    def val_steps_per_epoch(self):
        return 0

    def train_batch(self):
        self.i += 1
        return self.batches[self.i - 1]


def lfo_setup(dev, total=4):
    n, sr = 22272, 44100
    cfg = dict(in_ch=2, n_samples=n, sr=sr, n_fft=1024, hop_len=256, n_mels=64, kernel_size=(5, 13), out_channels=[64] * 6,
               temp_dilations=[1, 1, 2, 4, 8, 16], pool_size=(2, 1), latent_dim=1, use_ln=True)
    torch.manual_seed(1234); np.random.seed(1234)                     # same weights and same full batch everywhere
    module = lightning.LFOExtraction(models.Spectral2DCNN(**cfg), sr=sr, use_dry=True, model_smooth_n_frames=0,
                                     loss_dict={"l1": 1.0, "fdl1": 5.0, "sdl1": 10.0, "mse": 0.0}).to(dev).eval()
    opt = optim.FlatAdamW(module.parameters(), lr=1e-3, betas=(0.8, 0.99))
    g = torch.Generator().manual_seed(99)
    dry = torch.rand(total, 1, n, generator=g) * 1.6 - 0.8
    wet = (0.6 * dry + 0.3 * torch.roll(dry, 9, -1)).clamp(-1, 1)
    t = torch.arange(882) / 441.0
    mod = torch.stack([0.5 + 0.5 * torch.cos(2 * np.pi * (0.7 + 0.4 * i) * t + 0.3 * i) for i in range(total)])

    def batch(sl):
        return (dry[sl].to(dev), wet[sl].to(dev), mod[sl].to(dev), None)
    return module, opt, batch


def tbptt_setup(dev, total=4, **opt_kw):
    n = 5200
    torch.manual_seed(4321); np.random.seed(4321)
    em = models.LSTMEffectModel()
    module = lightning.TBPTTLFOEffectModeling(1024, 1024, em, lfo_model=None, model_smooth_n_frames=0, should_stretch=False,
                                              discard_invalid_lfos=False, loss_dict={"l1": 1.0, "esr": 0.0, "dc": 0.0}).to(dev).train()
    opt = optim.FlatAdamW(module.parameters(), lr=1e-3, betas=(0.8, 0.99), **opt_kw)
    g = torch.Generator().manual_seed(77)
    dry = torch.rand(total, 1, n, generator=g) * 1.6 - 0.8
    wet = (0.7 * dry + 0.2 * torch.roll(dry, 5, -1)).clamp(-1, 1)
    t = torch.arange(64) / 64.0
    mod = torch.stack([0.5 + 0.5 * torch.cos(2 * np.pi * (1.0 + 0.5 * i) * t + 0.4 * i) for i in range(total)])
    return module, opt, (dry.to(dev), wet.to(dev), mod.to(dev), None)


def fit_once(module, opt, batches, **trainer_kw):
    """One epoch of `Trainer.fit` over `batches`; returns the trainer."""
    t = trainer.Trainer(max_epochs=1, log_fn=None, **trainer_kw)
    t.fit(module, ListData(batches), opt)
    torch.cuda.synchronize()
    return t


def main() -> None:
    out_path, total, clip_val = sys.argv[1], int(sys.argv[2]), float(sys.argv[3])
    env = trainer.init_distributed()
    rank, world = env["rank"], env["world_size"]
    dev = torch.device("cuda", env["local_rank"])
    torch.cuda.set_device(dev)
    module, opt, batch = lfo_setup(dev, total)
    per = total // world
    fit_once(module, opt, [batch(slice(rank * per, (rank + 1) * per))], gradient_clip_val=clip_val)
    torch.save({"param": opt.flat_param.cpu(), "grad": opt.flat_grad.cpu() / world, "norm": opt.last_grad_norm.cpu(),
                "scale": opt.last_clip_scale.cpu(), "world": world, "steps": opt.step_count}, f"{out_path}.rank{rank}")
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()

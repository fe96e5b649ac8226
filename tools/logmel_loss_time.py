"""Timing of the log-mel L1 loss (mx_logmel_l1_loss) with HIP events, fixed seed.  Prints three lines:

  (a) value + gradient of one 128 x 1024 chunk (the config-4 TBPTT chunk)
  (b) value + gradient and value only on 256 x 88 200 clips, next to two mx_logmel_fwd calls on the same input (what the
      loss module evaluated before)
  (c) ms per config-4-shaped TBPTT batch (128 clips, warm-up 1024, 83 steps of 1024, LSTM-64, ground-truth LFO) with
      {"l1": 1, "log_mel_l1": 1} against {"l1": 1, "esr": 1}, both on the general effect_loss_grad path

    python tools/logmel_loss_time.py [--reps 20]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from mod_extraction_amd import lightning, losses, models, optim
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    mod = losses.LogMelLoss()
    mod.spectrogram.to(dev)

    x = torch.rand(128, 1024, device=dev) * 1.6 - 0.8
    y = (0.7 * x + 0.2 * torch.roll(x, 5, -1)).contiguous()
    ms_a = timed(lambda: losses.logmel_l1_value_and_grad(mod, x, y), args.reps)
    print(f"(a) 128 x 1024 chunk, value + gradient: {1e3 * ms_a:.1f} us")

    x = torch.rand(256, 88200, device=dev) * 1.6 - 0.8
    y = (0.7 * x + 0.2 * torch.roll(x, 5, -1)).contiguous()
    ms_g = timed(lambda: losses.logmel_l1_value_and_grad(mod, x, y), args.reps)
    ms_v = timed(lambda: losses.logmel_l1_value_and_grad(mod, x, y, need_grad=False), args.reps)
    n_frames = 1 + 88200 // 256
    pitch = -(-n_frames // 16) * 16
    sp = mod.spectrogram
    x3, y3 = x[:, None, :], y[:, None, :]
    ms_f = timed(lambda: (sp.log_mel(x3, n_frames, 1e-7, pitch=pitch), sp.log_mel(y3, n_frames, 1e-7, pitch=pitch)), args.reps)
    print(f"(b) 256 x 88200: value + gradient {ms_g:.3f} ms, value only {ms_v:.3f} ms, two mx_logmel_fwd {ms_f:.3f} ms")

    B, W, S, n = 128, 1024, 1024, 1024 + 83 * 1024
    dry = torch.rand(B, 1, n, device=dev) * 1.6 - 0.8
    wet = (0.7 * dry + 0.2 * torch.roll(dry, 5, -1)).clamp(-1, 1)
    lfo = torch.rand(B, 345, device=dev)
    res = {}
    for tag, ld in (("l1+log_mel_l1", {"l1": 1.0, "log_mel_l1": 1.0}), ("l1+esr", {"l1": 1.0, "esr": 1.0})):
        torch.manual_seed(1)
        em = models.LSTMEffectModel()
        step = lightning.TBPTTLFOEffectModeling(W, S, em, lfo_model=None, model_smooth_n_frames=0, should_stretch=False,
                                                discard_invalid_lfos=False, loss_dict=ld).to(dev).train()
        opt = optim.FlatAdamW(step.parameters(), lr=1e-4, betas=(0.8, 0.99))
        res[tag] = timed(lambda: step.common_step((dry, wet, lfo, None), is_training=True, optimizer=opt), max(2, args.reps // 10))
    r = res["l1+log_mel_l1"] / res["l1+esr"]
    print(f"(c) TBPTT batch (128 clips, 83 steps of 1024): l1+log_mel_l1 {res['l1+log_mel_l1']:.1f} ms, "
          f"l1+esr {res['l1+esr']:.1f} ms ({100 * (r - 1):+.1f} %)")


if __name__ == "__main__":
    main()

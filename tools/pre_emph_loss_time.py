"""Timing of the pre-emphasised ESR (mx_pre_emph_esr_grad) with HIP events, fixed seed: ``effect_loss_grad`` with
{"l1": 1, "esr_pre": 1} beside {"l1": 1, "esr": 1} in the same run, and the two gradient kernels on their own
(mx_pre_emph_esr_grad, Wright's taps [-0.95, 1], beside mx_effect_loss_grad with l1 + esr), on

  128 x 1024    the config-4 TBPTT chunk
  96 x 88 200   config 3's draw

Median of --rounds rounds of --launches calls each.

    python tools/pre_emph_loss_time.py [--rounds 5] [--launches 200] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, rounds, launches):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / launches)
    return statistics.median(ms), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from mod_extraction_amd import _hip, effect_losses, losses
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    mod = losses.PreEmphESRLoss()
    taps = mod.taps.on(dev)
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "launches": args.launches, "unit": "ms", "shapes": {}}
    for B, T in ((128, 1024), (96, 88200)):
        y = torch.rand(B, 1, T, device=dev) * 1.6 - 0.8
        y_hat = (0.7 * y + 0.2 * torch.roll(y, 5, -1)).contiguous()
        a, t = y_hat[:, 0, :], y[:, 0, :]
        dy, part = torch.empty((B, T), device=dev), torch.empty((B, 2), device=dev)
        cases = {
            "effect_loss_grad l1+esr_pre": lambda: effect_losses.effect_loss_grad(y_hat, y, {"l1": 1.0, "esr_pre": 1.0}, pre_emph=mod),
            "effect_loss_grad l1+esr": lambda: effect_losses.effect_loss_grad(y_hat, y, {"l1": 1.0, "esr": 1.0}),
            "mx_pre_emph_esr_grad": lambda: _hip.call("mx_pre_emph_esr_grad", a.data_ptr(), a.stride(0), t.data_ptr(), t.stride(0),
                                                      B, T, _hip.ptr(taps), 2, 0, 1.0, 1e-8, 0, _hip.ptr(part), _hip.ptr(dy),
                                                      dy.stride(0), _hip.stream()),
            "mx_effect_loss_grad l1+esr": lambda: _hip.call("mx_effect_loss_grad", a.data_ptr(), a.stride(0), t.data_ptr(),
                                                            t.stride(0), B, T, 1.0, 0.0, 1.0, 0.0, 1e-8, 0, _hip.ptr(dy),
                                                            dy.stride(0), _hip.stream()),
        }
        res = {}
        for name, fn in cases.items():
            med, ms = timed(fn, args.rounds, args.launches)
            res[name] = {"median": med, "rounds": ms}
            print(f"{B} x {T}: {name}: {1e3 * med:.1f} us  (rounds {', '.join(f'{1e3 * v:.1f}' for v in ms)})", flush=True)
        out["shapes"][f"{B}x{T}"] = res
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({k: {n: round(v["median"], 5) for n, v in s.items()} for k, s in out["shapes"].items()}))


if __name__ == "__main__":
    main()

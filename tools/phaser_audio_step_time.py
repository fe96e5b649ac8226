"""Timing of the low-rate LFO path of the phaser and of the training step built on it, with HIP events, fixed seed.

Shape: config 2's draw (configs/train_lfo_phaser.yml: 64 phaser clips x 2 s), as the step sees it: the batch's dry clips
(no lead-in), the label resampled to the extractor's frame rate (N // 256 + 1 = 345 points).

  expand     mx_phaser_mod_expand          (64, 345) -> (64, N / 4)
  forward    mx_phaser_fwd_stash           on the expanded row (the launch the step shares with fx.PhaserModule)
  backward   mx_phaser_bwd                 asked for dmod alone (no dx, no parameter sums), as the step asks
  gather     mx_phaser_dmod_gather         (64, N / 4) -> (64, 345)
  step       LFOExtractionThroughEffect(effect="phaser").audio_loss forward + backward for a free LFO: the four launches,
             the MR-STFT value-and-gradient kernels and the allocations in between

The five are timed alternately, --rounds times --reps launches each; the median round is reported with every round's
value.  The decision rule this tool serves (profiles/r10/README.md): if expand + gather together take longer than the
stash forward, fusing them into the scan is the follow-up.

The measurement runs in a child process under a time limit.

    python tools/phaser_audio_step_time.py [--reps 10] [--rounds 5] [--out profiles/r10/phaser_audio_step_time.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR = 44100
LIMIT = 300                                                                   # seconds, for the child


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternate(fns, reps, rounds):
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            t[k].append(timed(f, reps))
    return {k: {"median_ms": float(np.median(v)), "rounds_ms": [round(x, 4) for x in v]} for k, v in t.items()}


def measure(reps, rounds):
    from mod_extraction_amd import data_modules, fx, lightning
    from mod_extraction_amd.util import linear_interpolate_last_dim
    dev = torch.device("cuda:0")
    B, N = 64, 2 * SR
    torch.manual_seed(0)
    np.random.seed(0)
    bt = data_modules.SyntheticFxBatcher(B, N, SR, ("phaser",), dev, audio_seed=0, overlap=False)
    dry, wet, mod, fxp = bt.next_batch()
    step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect="phaser", audio_loss_dict={"mrstft": 1.0})
    x = dry[:, 0].contiguous()
    p = step.clip_constants(fxp, B, dev)
    lfo = linear_interpolate_last_dim(mod, N // 256 + 1, align_corners=True).contiguous()
    n_f = lfo.size(1)
    dy = torch.randn(B, N, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    mod_g = fx.phaser_mod_expand(lfo, None, N, N)
    y, st = fx.phaser_forward_stash(x, p, None, SR, N, mod=mod_g)
    dmod_g = torch.empty_like(mod_g)
    h = lfo.clone().requires_grad_(True)

    def run_step():
        h.grad = None
        step.audio_loss(h, dry, wet, fxp)[0].backward()

    fns = {"expand": lambda: fx.phaser_mod_expand(lfo, None, N, N, out=mod_g),
           "forward": lambda: fx.phaser_forward_stash(x, p, None, SR, N, mod=mod_g, out=y, stash=st),
           "backward": lambda: fx.phaser_backward(dy, x, st, p, None, SR, N, need_dx=False, params_wanted=(), dmod=dmod_g),
           "gather": lambda: fx.phaser_dmod_gather(dmod_g, None, N, n_f),
           "step": run_step}
    res = alternate(fns, reps, rounds)
    print(f"config 2 draw: {B} phaser clips x {N} samples, LFO {n_f} points")
    for k, v in res.items():
        print(f"  {k:9s} {v['median_ms']:.4f} ms   (rounds: {v['rounds_ms']})")
    extra = res["expand"]["median_ms"] + res["gather"]["median_ms"]
    fwd = res["forward"]["median_ms"]
    print(f"  expand + gather = {extra:.4f} ms = {extra / fwd:.3f} x the stash forward")
    return dict(res, clips=B, samples=N, lfo_points=n_f, expand_plus_gather_ms=round(extra, 4),
                expand_plus_gather_over_forward=round(extra / fwd, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the results as JSON")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(measure(args.reps, args.rounds)))
        return 0
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child",
           "--reps", str(args.reps), "--rounds", str(args.rounds)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    lines = p.stdout.splitlines()
    print("\n".join(l for l in lines if not l.startswith("RESULT ")), flush=True)
    if p.returncode != 0:
        print(f"exit status {p.returncode}")
        return p.returncode
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"reps": args.reps, "rounds": args.rounds, "config2": json.loads(
                next(l for l in lines if l.startswith("RESULT "))[7:])}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Timing of the differentiable phaser (mx_phaser_fwd_stash + mx_phaser_bwd) with HIP events, fixed seed.  Prints, for
config 3's phaser draw (the phaser rows of 256 interwoven clips x (2 s + lead)) and config 2's (64 phaser clips):

  (a) mx_phaser_fwd          the forward as the data modules launch it
  (b) the stash forward      same clips, built-in oscillator; ratio to (a) (extra stores only)
  (c) mx_phaser_bwd          dx, dmod and the four parameter gradients; ratio to (a)

The three are timed alternately, --rounds times --reps launches each, and the median round is reported.

    python tools/phaser_grad_time.py [--reps 10] [--rounds 5]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SR = 44100


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def draw(batch, effects, dev, seed):
    """The phaser rows of one batch of the synthetic batcher: source rows, per-clip parameters, leads."""
    from mod_extraction_amd import data_modules
    N = 2 * SR
    bt = data_modules.SyntheticFxBatcher(batch, N, SR, effects, dev, audio_seed=seed, overlap=False)
    _, _, _, d = bt.next_batch()
    idx = bt.rows_ph.long()
    src = bt.src[idx].contiguous()
    p = {k: d[k][idx].float().contiguous() for k in ("rate_hz", "depth", "centre_frequency_hz", "feedback", "mix")}
    lead = d["lead"][idx].to(torch.int32).contiguous()
    return src, p, lead, N


def measure(name, src, p, lead, N, reps, rounds):
    from mod_extraction_amd import fx
    B = src.size(0)
    y = torch.empty((B, N), device=src.device)
    y2, st = fx.phaser_forward_stash(src, p, lead, SR, N)
    fx.phaser_forward(src, p, lead, SR, N, out=y)
    assert torch.equal(y, y2)
    dy = torch.randn_like(y)
    dx = torch.empty_like(src)
    dmod = torch.empty((B, (src.size(1) + 3) // 4), device=src.device)
    fns = {"fwd": lambda: fx.phaser_forward(src, p, lead, SR, N, out=y),
           "stash": lambda: fx.phaser_forward_stash(src, p, lead, SR, N, out=y2, stash=st),
           "bwd": lambda: fx.phaser_backward(dy, src, st, p, lead, SR, N, dx=dx, dmod=dmod)}
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            t[k].append(timed(f, reps))
    med = {k: float(np.median(v)) for k, v in t.items()}
    samples = int((lead.long() + N).sum())
    print(f"{name}: {B} clips, {samples / B:.0f} processed samples per clip (lead included)")
    print(f"  (a) mx_phaser_fwd       {med['fwd']:.3f} ms   (rounds: {' '.join(f'{v:.3f}' for v in t['fwd'])})")
    print(f"  (b) stash forward       {med['stash']:.3f} ms = {med['stash'] / med['fwd']:.2f}x (a)   "
          f"(rounds: {' '.join(f'{v:.3f}' for v in t['stash'])})")
    print(f"  (c) mx_phaser_bwd       {med['bwd']:.3f} ms = {med['bwd'] / med['fwd']:.2f}x (a)   "
          f"(rounds: {' '.join(f'{v:.3f}' for v in t['bwd'])})")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    np.random.seed(0)
    measure("config 3 draw", *draw(256, ("flanger", "chorus", "phaser"), dev, 0), args.reps, args.rounds)
    torch.manual_seed(0)
    np.random.seed(0)
    measure("config 2 draw", *draw(64, ("phaser",), dev, 0), args.reps, args.rounds)


if __name__ == "__main__":
    main()

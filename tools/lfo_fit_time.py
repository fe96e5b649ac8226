"""Timing of the LFO fit (modulations.fit_lfo, csrc/lfo_fit.hip) with HIP events and the wall clock, fixed seed.  It claims
nothing until it has run: no figure of this tool is on record unless profiles/ holds its JSON.

  rows     256 x 345 and 64 x 345 points at 172.5 Hz (2 s clips), clean LFOs of the six default shapes at 0.5 .. 6 Hz with a
           little noise (sigma 0.02), rate window 0.25 .. 8 Hz
  grids    the default (rate_div 4, 32 phases: 63 x 32 coarse candidates a shape) and the fine one (rate_div 8, 64 phases:
           125 x 64), both with 4 refinement rounds
  times    --rounds rounds of --reps launches, the cases alternating within a round: per launch the HIP-event time and the
           wall-clock time (launches enqueued back to back, one synchronisation a round); the median round is reported
           with every round's value, and with it the template evaluations of the coarse grid over the event time -- a
           figure to compare runs by, not a roofline claim

The measurement runs in a child process under a time limit.

    python tools/lfo_fit_time.py [--reps 50] [--rounds 5] [--out profiles/r18/lfo_fit_time.json]
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT = 420                                                                   # seconds, for the child
N, SR, WINDOW = 345, 172.5, (0.25, 8.0)
GRIDS = {"default": {"rate_div": 4, "n_phases": 32}, "fine": {"rate_div": 8, "n_phases": 64}}


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, (time.perf_counter() - t0) * 1e3 / reps


def rows(B, dev):
    from mod_extraction_amd import modulations as M
    g = torch.Generator().manual_seed(B)
    freq = (0.5 + 5.5 * torch.rand(B, generator=g)).to(dev)
    phase = (2 * math.pi * torch.rand(B, generator=g)).to(dev)
    shape = torch.randint(0, 6, (B,), generator=g).to(torch.int32).to(dev)
    y = 0.1 + 0.7 * M.make_mod_signals(N, SR, freq, phase, shape)
    return (y + 0.02 * torch.randn(B, N, generator=g).to(dev)).contiguous()


def measure(args):
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    from mod_extraction_amd import modulations as M
    dev = torch.device("cuda:0")
    cases = {}
    for B in (256, 64):
        y = rows(B, dev)
        for name, grid in GRIDS.items():
            K = int(math.floor((WINDOW[1] - WINDOW[0]) * grid["rate_div"] * N / SR)) + 1
            cases[f"B{B}_{name}"] = (lambda y=y, grid=grid: M.fit_lfo(y, SR, WINDOW, **grid),
                                     {"rows": B, "points": N, "coarse_evaluations": 6 * K * grid["n_phases"] * N * B, **grid})
    for fn, _ in cases.values():
        fn()
    torch.cuda.synchronize()
    ev, wall = {k: [] for k in cases}, {k: [] for k in cases}
    for _ in range(args.rounds):
        for k, (fn, _) in cases.items():
            e, w = timed(fn, args.reps)
            ev[k].append(e)
            wall[k].append(w)
    out = {"device": torch.cuda.get_device_name(0), "cases": {}}
    for k, (_, info) in cases.items():
        med = float(np.median(ev[k]))
        out["cases"][k] = dict(info, event_median_ms=med, wall_median_ms=float(np.median(wall[k])),
                               event_rounds_ms=[round(x, 4) for x in ev[k]], wall_rounds_ms=[round(x, 4) for x in wall[k]],
                               coarse_gevals_per_s=info["coarse_evaluations"] / (med * 1e-3) / 1e9)
        print(f"  {k:13s} events {med:9.4f} ms   wall {out['cases'][k]['wall_median_ms']:9.4f} ms   coarse grid "
              f"{out['cases'][k]['coarse_gevals_per_s']:7.1f} G evaluations/s   (event rounds: {out['cases'][k]['event_rounds_ms']})")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the results as JSON")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(measure(args)))
        return 0
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps),
           "--rounds", str(args.rounds)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    lines = p.stdout.splitlines()
    print("\n".join(l for l in lines if not l.startswith("RESULT ")), flush=True)
    if p.returncode != 0:
        print(f"exit status {p.returncode}")
        return p.returncode
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(json.loads(next(l for l in lines if l.startswith("RESULT "))[7:]), reps=args.reps, rounds=args.rounds),
                      f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

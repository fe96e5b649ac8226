"""Timing of the loss warm-up window of lightning.LFOExtractionThroughEffect(warmup_ms=...) and of mx_lfo_stitch (K22) with HIP
events and the wall clock, fixed seed.  It claims nothing until it has run: no figure of this tool is on record unless
profiles/ holds its JSON.

  step     96 flanger clips of 2 s at 44.1 kHz from the batcher, {"mrstft": 1}, the LFO off the label, forward and backward of
           audio_loss: warmup_ms = None and 110, each without a match and with match_fir = 9.  The same launches run on views,
           so the expectation is "equal but for the shorter rows the losses see and one copy of dy without a match".
  stitch   file_eval.stitch_lfo on a 60 s recording (L = 2 646 000, windows of 88 200 at hop 44 100: 59 windows of 345 points,
           10 350 track points): one launch, stated as launch latency.
  times    --rounds rounds of --reps calls, the cases alternating within a round; the median round is reported with every
           round's value.

A tree without the feature (the parent commit) runs the cases it has: the tool asks the constructor's signature and the
package for file_eval.  The measurement runs in a child process under a time limit.

    python tools/warmup_step_time.py [--reps 5] [--rounds 5] [--out profiles/r23/warmup_step_time.json]
"""
import argparse
import inspect
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
LIMIT = 300                                                                   # seconds, for the child


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


def measure(args):
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    from mod_extraction_amd import data_modules, lightning
    dev = torch.device("cuda:0")
    has_warmup = "warmup_ms" in inspect.signature(lightning.LFOExtractionThroughEffect.__init__).parameters
    cases = {}
    Bs, Ns = 96, 88200
    torch.manual_seed(7)
    np.random.seed(7)
    batcher = data_modules.SyntheticFxBatcher(Bs, Ns, 44100, ("flanger",), dev, audio_seed=7, fixed_lead=0)
    dry, wet, mod, fxp = batcher.render(batcher.sample_params())
    t = torch.linspace(0.0, 1.0, mod.size(1), device=dev)
    h0 = (mod + 0.1 * torch.sin(2 * math.pi * 1.5 * t)[None, :]).clamp(0.0, 1.0).contiguous()
    for K in (None, 9):
        for ms in (None, 110.0) if has_warmup else (None,):
            kw = {} if ms is None else {"warmup_ms": ms}
            step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=44100, effect="flanger",
                                                        audio_loss_dict={"mrstft": 1.0}, match_fir=K, **kw).to(dev)

            def run(step=step):
                h = h0.clone().requires_grad_(True)
                loss, _ = step.audio_loss(h, dry, wet, fxp)
                loss.backward()

            cases[f"step_B{Bs}_N{Ns}_match_fir_{K}_warmup_ms_{ms}"] = (run, args.reps)
    try:
        from mod_extraction_amd import file_eval
    except ImportError:
        file_eval = None
    if file_eval is not None:
        L, N, n_f = 60 * 44100, 88200, 345
        starts = file_eval.window_starts(L, N)
        windows = torch.rand((len(starts), n_f), generator=torch.Generator().manual_seed(1)).to(dev)
        st = torch.tensor(starts, dtype=torch.int64, device=dev)
        out = torch.empty(file_eval.default_track_points(L, N, n_f), device=dev)
        cases[f"stitch_L{L}_W{len(starts)}_nt{out.numel()}"] = (lambda: file_eval.stitch_lfo(windows, st, L, N, out=out), 20 * args.reps)
    for fn, _ in cases.values():
        fn()
    torch.cuda.synchronize()
    ev, wall = {k: [] for k in cases}, {k: [] for k in cases}
    for _ in range(args.rounds):
        for k, (fn, reps) in cases.items():
            e, w = timed(fn, reps)
            ev[k].append(e)
            wall[k].append(w)
    res = {"device": torch.cuda.get_device_name(0), "has_warmup": has_warmup, "has_file_eval": file_eval is not None, "cases": {}}
    for k in cases:
        res["cases"][k] = {"event_median_ms": float(np.median(ev[k])), "wall_median_ms": float(np.median(wall[k])),
                           "event_rounds_ms": [round(x, 4) for x in ev[k]], "wall_rounds_ms": [round(x, 4) for x in wall[k]]}
        print(f"  {k:52s} events {res['cases'][k]['event_median_ms']:9.4f} ms   wall {res['cases'][k]['wall_median_ms']:9.4f} ms   "
              f"(event rounds: {res['cases'][k]['event_rounds_ms']})")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
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

"""Timing of the batched LFO variants (mx_lfo_quasi_periodic, mx_lfo_combined) beside the per-item loops they replace, at
the data path's size: 256 rows of 882 points, rates 0.5 - 3 Hz, S = 16 table entries per row.  For each of

  (a) modulations.make_quasi_periodic_batch      one launch
  (b) modulations.make_quasi_periodic            row by row (host RNG draws, corner indices pulled to the host, one
                                                 resampling launch per section)
  (c) modulations.make_combined_mod_sigs         one launch (synthesis of the base included)
  (d) modulations.make_combined_mod_sig          row by row (one synthesis launch per section)

it prints the HIP-event time and the host wall-clock time (both around work that ends in a device synchronise): median,
minimum and maximum over `--rounds` rounds of `--reps` calls, the batched and per-item forms alternating within a round.
The claim behind these kernels is the absence of host round trips, not a bandwidth figure: a row is 3.5 KB.  Nothing is
gated; this tool is how the numbers in profiles/r12/ are produced.

    python tools/lfo_variants_time.py [--rows 256] [--rounds 5] [--reps 200] [--item-reps 2] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = ["cos", "tri", "rect_cos", "inv_rect_cos", "saw", "rsaw"]


def timed(fn, reps):
    """(event ms, wall ms) per call of `reps` back-to-back calls, the device drained before and after"""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, (time.perf_counter() - t0) * 1e3 / reps


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--item-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from mod_extraction_amd import modulations as amod
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    np.random.seed(0)
    B, n, sr, S = args.rows, 882, 441.0, 16
    freq_h = torch.rand(B) * 2.5 + 0.5
    phase_h = torch.rand(B) * 6.28
    shape_h = torch.randint(0, len(SHAPES), (B,))
    freq, phase = freq_h.to(dev), phase_h.to(dev)
    shape = shape_h.to(torch.int32).to(dev)
    base = amod.make_mod_signals(n, sr, freq, phase, shape)
    shrink_h, amount_h = amod.draw_quasi_tables(B, S, 0.1, 0.3333, 0.1, 0.3333, 0.5)
    shrink, amount = shrink_h.to(dev), amount_h.to(dev)
    table = amod.draw_combined_table(B, S, SHAPES).to(dev)
    out = torch.empty_like(base)
    rows = [base[i].clone() for i in range(B)]

    def quasi_batch():
        amod.make_quasi_periodic_batch(base, shrink, amount, out=out)

    def quasi_items():
        for i in range(B):
            amod.make_quasi_periodic(rows[i], 0.1, 0.3333, 0.1, 0.3333, 0.5)

    def combined_batch():
        amod.make_combined_mod_sigs(n, sr, freq, phase, table)

    def combined_items():
        for i in range(B):
            amod.make_combined_mod_sig(n, sr, float(freq_h[i]), float(phase_h[i]), SHAPES, device=dev)

    work = {"quasi_batch": (quasi_batch, args.reps), "quasi_per_item": (quasi_items, args.item_reps),
            "combined_batch": (combined_batch, args.reps), "combined_per_item": (combined_items, args.item_reps)}
    for fn, _ in work.values():                                 # warm-up: code objects, allocator
        fn()
        fn()
    _, nc = amod.make_quasi_periodic_batch(base, shrink, amount)
    _, nb = amod.make_combined_mod_sigs(n, sr, freq, phase, table)
    res = {k: {"event_ms": [], "wall_ms": []} for k in work}
    for _ in range(args.rounds):
        for k, (fn, reps) in work.items():
            ev, wall = timed(fn, reps)
            res[k]["event_ms"].append(ev)
            res[k]["wall_ms"].append(wall)
    report = {"rows": B, "points": n, "S": S, "rounds": args.rounds, "reps": args.reps, "item_reps": args.item_reps,
              "mean_corners_quasi": float(nc.float().mean()), "max_corners_quasi": int(nc.max()),
              "mean_bottom_corners_combined": float(nb.float().mean()), "device": torch.cuda.get_device_name(0),
              "timings": {k: {m: summary(v) for m, v in r.items()} for k, r in res.items()}}
    for k, r in report["timings"].items():
        print(f"{k:18s} event {r['event_ms']['median']:9.4f} ms [{r['event_ms']['min']:.4f} .. {r['event_ms']['max']:.4f}]   "
              f"wall {r['wall_ms']['median']:9.4f} ms [{r['wall_ms']['min']:.4f} .. {r['wall_ms']['max']:.4f}]")
    t = report["timings"]
    for v in ("quasi", "combined"):
        print(f"{v}: per-item / batched wall-clock ratio {t[v + '_per_item']['wall_ms']['median'] / t[v + '_batch']['wall_ms']['median']:.0f}x")
    print(json.dumps(report))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()

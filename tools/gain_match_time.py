"""Timing of the gain match (mod_extraction_amd/gain.py, csrc/gain_match.hip) with HIP events and the wall clock, fixed seed.
It claims nothing until it has run: no figure of this tool is on record unless profiles/ holds its JSON.

  rows     96 x 88200 (a training batch of 2 s clips at 44.1 kHz) and 8 x 22272 (the tests' size): y_hat white noise, y a
           scaled y_hat plus 5 % noise, dz white noise
  cases    fwd        the forward pair of launches, mx_gain_match_partials + mx_gain_match_apply, into a preallocated z
           bwd        the backward pair, mx_gain_match_bwd_partials + mx_gain_match_bwd_apply, into a preallocated dy_hat
           torch_fwd  the same function ("ls", clamped) as torch expressions in the same process: fp32 elementwise products,
                      row sums, the gain, the clamp, the scaling
           torch_bwd  the same backward as torch expressions from saved g and a: the row sum of dz * y_hat, then the formula
           The torch route is the YARDSTICK: it is fp32 throughout (no fp64 sums, no fixed order), so it does less arithmetic;
           the file records both and whether the two launches of a direction are faster than it.
  times    --rounds rounds of --reps calls, the cases alternating within a round: per call the HIP-event time and the
           wall-clock time (calls enqueued back to back, one synchronisation a round); the median round is reported with
           every round's value, and the bytes a direction has to move over the event time

The measurement runs in a child process under a time limit.

    python tools/gain_match_time.py [--reps 20] [--rounds 5] [--out profiles/r21/gain_match_time.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT = 300                                                                   # seconds, for the child
SHAPES = ((96, 88200), (8, 22272))
EPS, LO, HI = 1e-8, 0.05, 20.0


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


def torch_fwd(p, q):
    a, c = (p * p).sum(1), (p * q).sum(1)
    g = (c / (a + EPS)).clamp(LO, HI)
    return g[:, None] * p, g, a


def torch_bwd(dz, p, q, g, a):
    k = ((dz * p).sum(1) / (a + EPS))[:, None]
    return g[:, None] * dz + k * (q - 2.0 * g[:, None] * p)


def measure(args):
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    from mod_extraction_amd import gain as G
    dev = torch.device("cuda:0")
    cases = {}
    for B, N in SHAPES:
        gen = torch.Generator().manual_seed(B)
        p = (0.25 * torch.randn(B, N, generator=gen)).to(dev)
        q = (0.5 * (p.cpu() + 0.0125 * torch.randn(B, N, generator=gen))).to(dev)
        dz = torch.randn(B, N, generator=gen).to(dev)
        z, dy = torch.empty_like(p), torch.empty_like(p)
        m = G.match_gain(p, q, "ls", EPS, (LO, HI), out=z)
        zt, gt, at = torch_fwd(p, q)
        d = G.match_gain_backward(dz, p, q, m, "ls", EPS, out=dy)
        dt = torch_bwd(dz, p, q, gt, at)
        assert int(m.flags.sum()) == 0
        info = {"rows": B, "samples": N,
                "fwd_max_rel_diff_to_torch": float(((z - zt).abs().max() / zt.abs().max()).cpu()),
                "bwd_max_rel_diff_to_torch": float(((d - dt).abs().max() / dt.abs().max()).cpu())}
        tag = f"B{B}_N{N}"
        cases[f"{tag}_fwd"] = (lambda p=p, q=q, z=z: G.match_gain(p, q, "ls", EPS, (LO, HI), out=z), dict(info, bytes=4 * 4 * B * N))
        cases[f"{tag}_bwd"] = (lambda dz=dz, p=p, q=q, m=m, dy=dy: G.match_gain_backward(dz, p, q, m, "ls", EPS, out=dy),
                               dict(info, bytes=6 * 4 * B * N))
        cases[f"{tag}_torch_fwd"] = (lambda p=p, q=q: torch_fwd(p, q), info)
        cases[f"{tag}_torch_bwd"] = (lambda dz=dz, p=p, q=q, gt=gt, at=at: torch_bwd(dz, p, q, gt, at), info)
    for fn, _ in cases.values():
        fn()
    torch.cuda.synchronize()
    ev, wall = {k: [] for k in cases}, {k: [] for k in cases}
    for _ in range(args.rounds):
        for k, (fn, _) in cases.items():
            e, w = timed(fn, args.reps)
            ev[k].append(e)
            wall[k].append(w)
    out = {"device": torch.cuda.get_device_name(0), "cases": {}, "faster_than_torch": {}}
    for k, (_, info) in cases.items():
        med = float(np.median(ev[k]))
        row = dict(info, event_median_ms=med, wall_median_ms=float(np.median(wall[k])),
                   event_rounds_ms=[round(x, 4) for x in ev[k]], wall_rounds_ms=[round(x, 4) for x in wall[k]])
        if "bytes" in info:
            row["gbytes_per_s"] = info["bytes"] / (med * 1e-3) / 1e9
        out["cases"][k] = row
        print(f"  {k:26s} events {med:9.4f} ms   wall {row['wall_median_ms']:9.4f} ms   (event rounds: {row['event_rounds_ms']})")
    for B, N in SHAPES:
        for way in ("fwd", "bwd"):
            mine, ref = out["cases"][f"B{B}_N{N}_{way}"], out["cases"][f"B{B}_N{N}_torch_{way}"]
            verdict = {"events": mine["event_median_ms"] < ref["event_median_ms"], "wall": mine["wall_median_ms"] < ref["wall_median_ms"]}
            out["faster_than_torch"][f"B{B}_N{N}_{way}"] = verdict
            print(f"  B{B}_N{N}_{way}: the two launches are {'FASTER' if verdict['events'] else 'NOT faster'} than the torch route by "
                  f"events, {'FASTER' if verdict['wall'] else 'NOT faster'} by the wall clock")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
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

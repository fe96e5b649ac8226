"""Timing of the rate contour (K25: rate_track.fit_rate_track, csrc/rate_track.hip) with HIP events and the wall clock, fixed
seed -- the sibling of tools/track_fit_time.py.  It claims nothing until it has run: no figure of this tool is on record unless
profiles/ holds its JSON.

  tracks     10 350 points (60 s) and 103 500 points (10 min) at 172.5 Hz: a triangle whose rate glides 1.0 -> 1.3 Hz with a
             little noise (sigma 0.02), slices of 690 points every 345, the default window 0.25 .. 8 Hz (K = 125, 4000 states a
             slice), six shapes, the default path
  launches   ``mx_rate_track_nodes`` (the statistics pre-pass and the node launch), ``mx_rate_track_path`` (the walk and the
             pick) and ``mx_rate_track_refine`` timed one by one on buffers made once, and ``fit_rate_track`` as a caller runs it
             (the plan, ``torch.empty`` and the three enqueues)
  slices     the same slices as ONE ``fit_lfo`` launch on a strided view (``as_strided``, one row a slice; the right-aligned last
             slice left out): independent fits, what a caller could do before.  A comparison of cost, not of function
  times      --rounds rounds of --reps calls (a tenth, at least one, on the 10 min track); per call the HIP-event time and the
             wall-clock time (calls enqueued back to back, one synchronisation a round); the median round is reported with every
             round's value, and for the node launch the template evaluations over the event time -- a figure to compare runs
             by, not a roofline claim

The measurement runs in a child process under a time limit.

    python tools/rate_track_time.py [--reps 20] [--rounds 5] [--out profiles/r27/rate_track_time.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.lfo_fit_time import timed                                          # noqa: E402  (the same event / wall-clock bracket)

LIMIT = 420                                                                   # seconds, for the child
SR, W, HOP, WINDOW, J, L, D = 172.5, 690, 345, (0.25, 8.0), 32, 4, 2


def track(n, dev):
    """A triangle gliding 1.0 -> 1.3 Hz over the row, noise 0.02: (1, n) fp32 on the device."""
    t = np.arange(1, n + 1) / SR
    cyc = np.cumsum(1.0 + 0.3 * (t - t[0]) / (t[-1] - t[0])) / SR
    saw = np.mod(cyc, 1.0)
    y = 0.1 + 0.7 * np.where(2 * saw > 1, 2 - 2 * saw, 2 * saw) + np.random.default_rng(n).normal(0.0, 0.02, n)
    return torch.from_numpy(y.astype(np.float32)).to(dev).view(1, n)


def launches(y):
    """The three enqueues on buffers made once: {name: callable}."""
    from mod_extraction_amd import _hip
    from mod_extraction_amd.file_eval import window_starts
    n, dev = y.size(1), y.device
    starts = torch.tensor(window_starts(n, W, HOP), dtype=torch.int64, device=dev)
    S = starts.numel()
    grid = (WINDOW[0], WINDOW[1], 0x3F, 4, J)
    sizes = (ctypes.c_int64 * 3)()
    a = ctypes.addressof(sizes)
    _hip.call("mx_rate_track_plan", 1, n, SR, S, W, *grid, L, D, a, a + 8, a + 16)
    node = torch.empty(sizes[1] // 8, device=dev, dtype=torch.float64)
    ws = torch.empty(sizes[2] // 8, device=dev, dtype=torch.float64)
    buf = (node.data_ptr(), sizes[1], ws.data_ptr(), sizes[2])
    i32 = lambda *s: torch.empty(s, device=dev, dtype=torch.int32)
    f32 = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)
    shape, gk, gj, cost, per = i32(1), i32(1, S), i32(1, S), f32(1), f32(1, 7)
    fitted = [f32(1, S) for _ in range(5)]
    st = _hip.stream
    return S, sizes[0], {
        "nodes": lambda: _hip.call("mx_rate_track_nodes", y.data_ptr(), n, 1, n, SR, starts.data_ptr(), S, W, *grid, *buf, st()),
        "path": lambda: _hip.call("mx_rate_track_path", 1, n, SR, starts.data_ptr(), S, W, *grid, D, 0.002, 1.0, *buf,
                                  shape.data_ptr(), gk.data_ptr(), gj.data_ptr(), cost.data_ptr(), per.data_ptr(), st()),
        "refine": lambda: _hip.call("mx_rate_track_refine", y.data_ptr(), n, 1, n, SR, starts.data_ptr(), S, W, *grid, L,
                                    shape.data_ptr(), gk.data_ptr(), gj.data_ptr(), *[o.data_ptr() for o in fitted], buf[2], buf[3],
                                    st())}


def measure(args):
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    from mod_extraction_amd import modulations as M, rate_track as R
    dev = torch.device("cuda:0")
    cases = {}
    for n in (10350, 103500):
        y = track(n, dev)
        S, K, fns = launches(y)
        assert (S, K) == R.rate_track_plan(n, SR, W, HOP)
        reps = args.reps if n < 100000 else max(1, args.reps // 10)
        info = {"points": n, "slices": S, "K": K}
        for name, fn in fns.items():                                          # in this order: each reads what the one before wrote
            extra = {"node_evaluations": 6 * S * K * J * W} if name == "nodes" else {}
            cases[f"{n}_{name}"] = (fn, dict(info, **extra), reps)
        cases[f"{n}_fit_rate_track"] = (lambda y=y: R.fit_rate_track(y, SR, W, HOP), info, reps)
        regular = (n - W) // HOP + 1
        view = torch.as_strided(y, (regular, W), (HOP, 1))
        assert M.fit_plan(W, SR) == ("lfo_fit", K)
        cases[f"{n}_independent_fit_lfo"] = (lambda v=view: M.fit_lfo(v, SR), dict(info, rows=regular), reps)
    for fn, _, _ in cases.values():
        fn()
    torch.cuda.synchronize()
    ev, wall = {k: [] for k in cases}, {k: [] for k in cases}
    for _ in range(args.rounds):
        for k, (fn, _, reps) in cases.items():
            e, w = timed(fn, reps)
            ev[k].append(e)
            wall[k].append(w)
    out = {"device": torch.cuda.get_device_name(0), "cases": {}}
    for k, (_, info, reps) in cases.items():
        med = float(np.median(ev[k]))
        row = dict(info, reps=reps, event_median_ms=med, wall_median_ms=float(np.median(wall[k])),
                   event_rounds_ms=[round(x, 4) for x in ev[k]], wall_rounds_ms=[round(x, 4) for x in wall[k]])
        if "node_evaluations" in info:
            row["node_gevals_per_s"] = info["node_evaluations"] / (med * 1e-3) / 1e9
        out["cases"][k] = row
        rate = f"   {row['node_gevals_per_s']:7.1f} G evaluations/s" if "node_gevals_per_s" in row else ""
        print(f"  {k:30s} events {med:10.4f} ms   wall {row['wall_median_ms']:10.4f} ms{rate}   (event rounds: "
              f"{row['event_rounds_ms']})")
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
            json.dump(dict(json.loads(next(l for l in lines if l.startswith("RESULT "))[7:]), rounds=args.rounds), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

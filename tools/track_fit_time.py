"""Timing of the track fit (K23: modulations.fit_lfo beyond K18's limits, csrc/track_fit.hip) with HIP events and the wall
clock, fixed seed -- the sibling of tools/lfo_fit_time.py.  It claims nothing until it has run: no figure of this tool is on
record unless profiles/ holds its JSON.

  both     ONE row of 4096 points at 172.5 Hz (a 0.55 Hz triangle), window 0.5 .. 0.6 Hz (K = 10: 320 coarse candidates a
           shape), six shapes -- the long shape both paths accept: ``mx_lfo_fit`` (K18, the yardstick) against ``mx_track_fit``
           called directly on the same row, the two alternating within a round
  tracks   10 350 points (60 s) and 103 500 points (10 min) of a 1.3 Hz triangle with a little noise (sigma 0.02), the default
           window 0.25 .. 8 Hz, six shapes, the default grid: ``fit_lfo``, i.e. the plan, the workspace from ``torch.empty``
           and the four launches
  times    --rounds rounds of --reps calls (a tenth of them, at least one, on the 10 min track); per call the HIP-event time
           and the wall-clock time (calls enqueued back to back, one synchronisation a round); the median round is reported with
           every round's value and the coarse grid's template evaluations over the event time -- a figure to compare runs by,
           not a roofline claim

The measurement runs in a child process under a time limit.

    python tools/track_fit_time.py [--reps 20] [--rounds 5] [--out profiles/r25/track_fit_time.json]
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
SR = 172.5


def track(n, rate, dev, noise):
    from mod_extraction_amd import modulations as M
    one = lambda v, dt=torch.float32: torch.tensor([v], dtype=dt, device=dev)
    y = 0.1 + 0.7 * M.make_mod_signals(n, SR, one(rate), one(1.0), one(3, torch.int32))
    g = torch.Generator().manual_seed(n)
    return (y + noise * torch.randn(1, n, generator=g).to(dev)).contiguous()


def direct(y, window):
    """``mx_track_fit`` on a row ``fit_lfo`` would hand to K18: buffers made once, one call a repetition."""
    from mod_extraction_amd import _hip
    n, dev = y.size(1), y.device
    grid = (SR, window[0], window[1], 0x3F, 4, 32, 4)
    sizes = (ctypes.c_int64 * 2)()
    _hip.call("mx_track_fit_plan", 1, n, *grid, ctypes.addressof(sizes), ctypes.addressof(sizes) + 8)
    ws = torch.empty(sizes[1] // 8, device=dev, dtype=torch.float64)
    outs = [torch.empty(1, device=dev, dtype=torch.int32)] + [torch.empty(1, device=dev, dtype=torch.float32) for _ in range(5)]
    return lambda: _hip.call("mx_track_fit", y.data_ptr(), n, 1, n, *grid, *[o.data_ptr() for o in outs], None, ws.data_ptr(),
                             sizes[1], _hip.stream())


def measure(args):
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    from mod_extraction_amd import modulations as M
    dev = torch.device("cuda:0")
    cases = {}
    y = track(4096, 0.55, dev, 0.0)
    both = (0.5, 0.6)
    assert M.fit_plan(4096, SR, both) == ("lfo_fit", 10)
    info = {"points": 4096, "K": 10, "coarse_evaluations": 6 * 10 * 32 * 4096}
    cases["both_4096_lfo_fit"] = (lambda y=y: M.fit_lfo(y, SR, both), info, args.reps)
    cases["both_4096_track_fit"] = (direct(y, both), info, args.reps)
    for n in (10350, 103500):
        y = track(n, 1.3, dev, 0.02)
        route, K = M.fit_plan(n, SR)
        assert route == "track_fit"
        cases[f"track_{n}"] = (lambda y=y: M.fit_lfo(y, SR), {"points": n, "K": K, "coarse_evaluations": 6 * K * 32 * n},
                               args.reps if n < 100000 else max(1, args.reps // 10))
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
        out["cases"][k] = dict(info, reps=reps, event_median_ms=med, wall_median_ms=float(np.median(wall[k])),
                               event_rounds_ms=[round(x, 4) for x in ev[k]], wall_rounds_ms=[round(x, 4) for x in wall[k]],
                               coarse_gevals_per_s=info["coarse_evaluations"] / (med * 1e-3) / 1e9)
        print(f"  {k:20s} events {med:10.4f} ms   wall {out['cases'][k]['wall_median_ms']:10.4f} ms   coarse grid "
              f"{out['cases'][k]['coarse_gevals_per_s']:7.1f} G evaluations/s   (event rounds: {out['cases'][k]['event_rounds_ms']})")
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

"""Timing of the warp (K26: alignment.warp_rows, csrc/warp.hip) and of the drift estimate with HIP events and the wall clock,
fixed seed -- the sibling of tools/resample_time.py.  It claims nothing until it has run: no figure of this tool is on record
unless profiles/ holds its JSON.

  cases    the default filter (half 51, 103 taps an output), offset 37.4, drift 3e-4: ONE row of 2 646 000 samples (a 60 s file)
           and 8 rows of 132 300 (3 s); unit-normal noise
  kernel   ``mx_warp_rows`` called directly, buffers and parameter arrays made once
  beta0    the same launch with beta = 0: the Kaiser window is 1 and its I0 series ends after one term, so the difference
           from ``kernel`` is what the series costs -- the elimination that says which part of the tap bounds the kernel
  torch    the same function as a torch expression on the same device, in fp64, in chunks of 65 536 outputs: positions,
           ``torch.sinc``, ``torch.special.i0``, a gather of the 103 samples and a sum -- for scale; its largest difference
           from the kernel's output is reported, no ratio is claimed
  estimate ``alignment.estimate_file_drift`` on a 60 s pair of white noise at +100 ppm with 16 probes of 8192 points, max_lag 2205 (50 ms): K19's two
           launches on 16 x 8192, the ``.cpu()`` and the host fit -- wall clock only (it synchronises)
  times    --rounds rounds of --reps calls; per call the HIP-event time and the wall-clock time (calls enqueued back to back,
           one synchronisation a round); the median round with every round's value, and from the event time the taps
           evaluated a second and the compulsory HBM traffic (x once, y once)

The measurement runs in a child process under a time limit.

    python tools/warp_time.py [--reps 5] [--rounds 5] [--out profiles/r28/warp_time.json]
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
from tools.lfo_fit_time import timed                                          # noqa: E402  (the same event / wall-clock bracket)

LIMIT = 300                                                                   # seconds, for the child
SHAPES = ((1, 2646000), (8, 132300))
OFFSET, DRIFT = 37.4, 3e-4
EST_DRIFT = 1e-4                                                              # of the pair the estimate is timed on
HALF, TAPS, C, BETA = 51, 103, 0.95, 16.0


def torch_form(x, offset, drift, n_out, chunk=65536):
    """The warp of every row of ``x`` along one line as a torch expression in fp64 (see the module docstring)."""
    B, n_in = x.shape
    xd = torch.nn.functional.pad(x.double(), (0, 1))                          # index n_in: the zero outside the row
    k = torch.arange(TAPS, device=x.device)
    j = (HALF - k).double()
    i0b = torch.special.i0(torch.tensor(BETA, dtype=torch.float64, device=x.device))
    out = torch.empty((B, n_out), device=x.device, dtype=torch.float32)
    for m0 in range(0, n_out, chunk):
        m = torch.arange(m0, min(n_out, m0 + chunk), device=x.device, dtype=torch.float64)
        pos = m + (m * drift + offset)
        fl = torch.floor(pos)
        tau = (pos - fl)[:, None] + j[None, :]
        r = (tau / HALF).clamp(-1.0, 1.0)
        h = C * torch.sinc(C * tau) * torch.special.i0(BETA * torch.sqrt(1.0 - r * r)) / i0b
        h = torch.where(tau.abs() <= HALF, h, torch.zeros_like(h))
        idx = fl.long()[:, None] - HALF + k[None, :]
        idx = torch.where((idx >= 0) & (idx < n_in), idx, torch.full_like(idx, n_in))
        out[:, m0:m0 + len(m)] = (xd[:, idx] * h[None]).sum(-1).float()
    return out


def measure(args):
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    from mod_extraction_amd import _hip, alignment
    dev = torch.device("cuda:0")
    cases, info = {}, {}
    for B, n in SHAPES:
        g = torch.Generator().manual_seed(n)
        x = torch.randn(B, n, generator=g).to(dev)
        y = torch.empty(B, n, device=dev)
        off = torch.full((B,), OFFSET, device=dev, dtype=torch.float64)
        dr = torch.full((B,), DRIFT, device=dev, dtype=torch.float64)
        key = f"{B}x{n}"

        def launch(beta, x=x, y=y, off=off, dr=dr, B=B, n=n):
            _hip.call("mx_warp_rows", x.data_ptr(), n, B, n, off.data_ptr(), dr.data_ptr(), None, 48, C, beta, y.data_ptr(), n, n,
                      _hip.stream())

        cases[key + "_kernel"] = lambda launch=launch: launch(BETA)
        cases[key + "_kernel_beta0"] = lambda launch=launch: launch(0.0)
        cases[key + "_torch_fp64"] = lambda x=x, n=n: torch_form(x, OFFSET, DRIFT, n)
        launch(BETA)
        diff = float((torch_form(x, OFFSET, DRIFT, n) - y).abs().max())
        for k in (key + "_kernel", key + "_kernel_beta0", key + "_torch_fp64"):
            info[k] = {"rows": B, "n_in": n, "n_out": n, "taps": TAPS, "max_abs_kernel_minus_torch": diff}
    torch.cuda.synchronize()
    ev, wall = {k: [] for k in cases}, {k: [] for k in cases}
    for _ in range(args.rounds):
        for k, fn in cases.items():
            e, w = timed(fn, 1 if k.endswith("torch_fp64") else args.reps)
            ev[k].append(e)
            wall[k].append(w)
    out = {"device": torch.cuda.get_device_name(0), "library": _hip.SO_PATH, "cases": {}}
    for k in cases:
        med = float(np.median(ev[k]))
        i = info[k]
        taps = i["rows"] * i["n_out"] * i["taps"]
        out["cases"][k] = dict(i, reps=1 if k.endswith("torch_fp64") else args.reps, event_median_ms=med,
                               wall_median_ms=float(np.median(wall[k])), event_rounds_ms=[round(v, 4) for v in ev[k]],
                               wall_rounds_ms=[round(v, 4) for v in wall[k]], gtaps_per_s=taps / (med * 1e-3) / 1e9,
                               hbm_gb_per_s=4 * i["rows"] * (i["n_in"] + i["n_out"]) / (med * 1e-3) / 1e9)
        c = out["cases"][k]
        print(f"  {k:28s} events {med:10.4f} ms   wall {c['wall_median_ms']:10.4f} ms   {c['gtaps_per_s']:8.2f} G taps/s   "
              f"HBM {c['hbm_gb_per_s']:7.1f} GB/s   |kernel - torch| {i['max_abs_kernel_minus_torch']:.2e}")
    # the estimate: wall clock, it ends in a .cpu()
    n = SHAPES[0][1]
    dry = torch.randn(n, generator=torch.Generator().manual_seed(1)).to(dev)
    wet = alignment.warp_rows(dry, -OFFSET / (1 + EST_DRIFT), 1 / (1 + EST_DRIFT) - 1)
    est = alignment.estimate_file_drift(dry, wet, 2205)
    torch.cuda.synchronize()
    walls = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        for _ in range(args.reps):
            alignment.estimate_file_drift(dry, wet, 2205)
        walls.append((time.perf_counter() - t0) / args.reps * 1e3)
    out["estimate_file_drift_16x8192"] = {"wall_median_ms": float(np.median(walls)), "wall_rounds_ms": [round(v, 4) for v in walls],
                                          "max_lag": 2205, "estimate": list(est), "true": [OFFSET, EST_DRIFT]}
    print(f"  estimate_file_drift 16 x 8192, max_lag 2205: wall {np.median(walls):.4f} ms; found {est.offset:.4f} + {1e6 * est.drift:.3f} ppm "
          f"(true {OFFSET} + {1e6 * EST_DRIFT:.0f} ppm), ok {est.ok}")
    return out


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
            json.dump(dict(json.loads(next(l for l in lines if l.startswith("RESULT "))[7:]), rounds=args.rounds), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

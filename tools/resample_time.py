"""Timing of the rational resampler (K24: resample.resample_rows, csrc/resample.hip) with HIP events and the wall clock, fixed
seed -- the sibling of tools/track_fit_time.py.  It claims nothing until it has run: no figure of this tool is on record unless
profiles/ holds its JSON.

  cases    48 000 -> 44 100 Hz with the default filter (up 147, down 160, 111 taps a phase): ONE row of 2 880 000 samples (a 60 s
           file) and 96 rows of 96 000 (a batch of 2 s clips); unit-normal noise
  kernel   ``mx_resample_rows`` called directly, buffers and the tap table made once -- the route is the loaded library's
           (``MODEX_HIP_LIB`` selects a build; one compiled with ``-DMX_RESAMPLE_LDS_TABLE_BYTES=0`` takes the L2 route at every
           ratio), and is reported
  torch    the same function as a torch expression on the same device: ``conv1d`` of the zero-padded rows with ``up`` output
           channels (channel r holds the phase of the outputs j up + r at its offset floor(r down / up)), stride ``down``, and the
           (B, up, J) result interleaved -- fp32 accumulation; its largest difference from the kernel's output is reported
  times    --rounds rounds of --reps calls; per call the HIP-event time and the wall-clock time (calls enqueued back to back,
           one synchronisation a round); the median round with every round's value, and from the event time the rates the
           kernel reached: fp64 FMAs, tap reads (4 bytes each: LDS on the LDS route), and the compulsory HBM traffic
           (x once, y once)

The measurement runs in a child process under a time limit.

    python tools/resample_time.py [--reps 20] [--rounds 5] [--out profiles/r26/resample_time_lds.json]
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
from tools.lfo_fit_time import timed                                          # noqa: E402  (the same event / wall-clock bracket)

LIMIT = 300                                                                   # seconds, for the child
SR_IN, SR_OUT = 48000, 44100
SHAPES = ((1, 2880000), (96, 96000))


def conv_form(plan, table):
    """``f(x) -> y``: the resampler as ``conv1d`` (see the module docstring)."""
    import torch.nn.functional as F
    up, down, half, T = plan.up, plan.down, plan.half, plan.taps_per_phase
    w = torch.zeros((up, 1, T + down - 1), device=table.device)
    for r in range(up):
        o, p = divmod(r * down, up)
        w[r, 0, o:o + T] = table[p]

    def f(x):
        B, n = x.shape
        n_out = plan.out_length(n)
        J = -(-n_out // up)
        need = (J - 1) * down + T + down - 1                    # padded length the last window reaches
        xp = F.pad(x, (half, max(0, need - half - n)))
        y = F.conv1d(xp[:, None, :], w, stride=down)[:, :, :J]
        return y.transpose(1, 2).reshape(B, J * up)[:, :n_out]

    return f


def measure(args):
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    from mod_extraction_amd import _hip, resample
    dev = torch.device("cuda:0")
    plan = resample.resample_plan(SR_IN, SR_OUT)
    table = plan.taps(dev)
    conv = conv_form(plan, table)
    cases, info = {}, {}
    for B, n in SHAPES:
        g = torch.Generator().manual_seed(n)
        x = torch.randn(B, n, generator=g).to(dev)
        n_out = plan.out_length(n)
        y = torch.empty(B, n_out, device=dev)
        key = f"{B}x{n}"
        cases[key + "_kernel"] = lambda x=x, y=y, B=B, n=n, n_out=n_out: _hip.call(
            "mx_resample_rows", x.data_ptr(), n, B, n, plan.up, plan.down, plan.half, table.data_ptr(), y.data_ptr(), n_out, n_out,
            _hip.stream())
        cases[key + "_torch_conv1d"] = lambda x=x: conv(x)
        cases[key + "_kernel"]()
        diff = float((conv(x) - y).abs().max())
        for k in (key + "_kernel", key + "_torch_conv1d"):
            info[k] = {"rows": B, "n_in": n, "n_out": n_out, "taps_per_phase": plan.taps_per_phase,
                       "max_abs_kernel_minus_conv1d": diff}
    torch.cuda.synchronize()
    ev, wall = {k: [] for k in cases}, {k: [] for k in cases}
    for _ in range(args.rounds):
        for k, fn in cases.items():
            e, w = timed(fn, args.reps)
            ev[k].append(e)
            wall[k].append(w)
    out = {"device": torch.cuda.get_device_name(0), "route": plan.route, "library": _hip.SO_PATH, "cases": {}}
    for k in cases:
        med = float(np.median(ev[k]))
        i = info[k]
        macs = i["rows"] * i["n_out"] * i["taps_per_phase"]
        out["cases"][k] = dict(i, reps=args.reps, event_median_ms=med, wall_median_ms=float(np.median(wall[k])),
                               event_rounds_ms=[round(v, 4) for v in ev[k]], wall_rounds_ms=[round(v, 4) for v in wall[k]],
                               gfma_per_s=macs / (med * 1e-3) / 1e9, tap_read_tb_per_s=4 * macs / (med * 1e-3) / 1e12,
                               hbm_gb_per_s=4 * i["rows"] * (i["n_in"] + i["n_out"]) / (med * 1e-3) / 1e9)
        c = out["cases"][k]
        print(f"  {k:28s} route {plan.route:3s}  events {med:9.4f} ms   wall {c['wall_median_ms']:9.4f} ms   {c['gfma_per_s']:8.1f} G FMA/s   "
              f"taps {c['tap_read_tb_per_s']:6.2f} TB/s   HBM {c['hbm_gb_per_s']:7.1f} GB/s   |kernel - conv1d| {i['max_abs_kernel_minus_conv1d']:.2e}")
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

"""Timing of the pair alignment (mod_extraction_amd/alignment.py, csrc/pair_align.hip) with HIP events and the wall clock,
fixed seed.  It claims nothing until it has run: no figure of this tool is on record unless profiles/ holds its JSON.

  rows     8 x 88200 (the probes of one file: 2 s chunks at 44.1 kHz) and 64 x 88200 (a row budget's worth), white noise
           through a comb, every row late by its own lag; L = 2205 (50 ms)
  launches mx_pair_xcorr, mx_pair_peak (on the r of the first) and mx_pair_shift, each on its own, and as context a
           cross-correlation of the same rows by torch's FFT in the same process (rfft of both rows zero-padded to
           2 N, a product, irfft, the 2 L + 1 lags gathered: fp32, so no like-for-like of the fp64 sums)
  times    --rounds rounds of --reps launches, the cases alternating within a round: per launch the HIP-event time and the
           wall-clock time (launches enqueued back to back, one synchronisation a round); the median round is reported
           with every round's value, and for xcorr the products over the event time -- a figure to compare runs by

The measurement runs in a child process under a time limit.

    python tools/pair_align_time.py [--reps 20] [--rounds 5] [--out profiles/r20/pair_align_time.json]
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
LIMIT = 420                                                                   # seconds, for the child
N, L = 88200, 2205


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
    g = torch.Generator().manual_seed(B)
    x = 0.25 * torch.randn(B, N + 2 * L + 64, generator=g)
    y = x.clone()
    y[:, 30:] += 0.5 * x[:, :-30]
    lags = torch.randint(-L, L + 1, (B,), generator=g)
    dry = x[:, 64 + L:64 + L + N].contiguous()
    wet = torch.stack([y[b, 64 + L - int(lags[b]):64 + L - int(lags[b]) + N] for b in range(B)])
    return dry.to(dev), wet.to(dev), lags


def fft_xcorr(dry, wet):
    n = 2 * N
    r = torch.fft.irfft(torch.fft.rfft(wet, n) * torch.fft.rfft(dry, n).conj(), n)
    return torch.cat([r[:, n - L:], r[:, :L + 1]], dim=1)


def measure(args):
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    from mod_extraction_amd import _hip, alignment as A
    dev = torch.device("cuda:0")
    cases = {}
    for B in (8, 64):
        dry, wet, lags = rows(B, dev)
        est = A.estimate_pair_lag(dry, wet, L)
        assert est.lag.cpu().tolist() == lags.tolist(), "the rows' own lags are not recovered"
        r = A.xcorr_lags(dry, wet, L)
        ref = fft_xcorr(dry, wet).double()
        rel = float(((r - ref).abs().max() / r.abs().max()).cpu())
        outs = (torch.empty_like(est.lag), torch.empty_like(est.corr), torch.empty_like(est.frac))
        shifted = torch.empty_like(wet)
        info = {"rows": B, "samples": N, "max_lag": L}
        cases[f"B{B}_xcorr"] = (lambda dry=dry, wet=wet: A.xcorr_lags(dry, wet, L),
                                dict(info, products=B * (2 * L + 1) * N, fft_max_rel_diff=rel))
        cases[f"B{B}_peak"] = (lambda dry=dry, wet=wet, r=r, outs=outs, B=B: _hip.call(
            "mx_pair_peak", dry.data_ptr(), N, wet.data_ptr(), N, r.data_ptr(), B, N, L, *[o.data_ptr() for o in outs],
            _hip.stream()), info)
        cases[f"B{B}_shift"] = (lambda wet=wet, est=est, shifted=shifted: A.shift_rows(wet, est.lag, est.corr, out=shifted),
                                dict(info, bytes=2 * 4 * B * N))
        cases[f"B{B}_torch_fft"] = (lambda dry=dry, wet=wet: fft_xcorr(dry, wet), info)
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
        row = dict(info, event_median_ms=med, wall_median_ms=float(np.median(wall[k])),
                   event_rounds_ms=[round(x, 4) for x in ev[k]], wall_rounds_ms=[round(x, 4) for x in wall[k]])
        if "products" in info:
            row["gproducts_per_s"] = info["products"] / (med * 1e-3) / 1e9
        if "bytes" in info:
            row["gbytes_per_s"] = info["bytes"] / (med * 1e-3) / 1e9
        out["cases"][k] = row
        print(f"  {k:14s} events {med:9.4f} ms   wall {row['wall_median_ms']:9.4f} ms   (event rounds: {row['event_rounds_ms']})")
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

"""Cost of gradient clipping on the optimizer launch, beside the un-clipped step of the same run, at the two parameter counts
the project trains: 1 340 353 (the LFO extractor) and 17 473 (the LSTM-64 under truncated BPTT, whose gradient arrives as one
row per clip: `--rows`).  For each size it times, with HIP events,

  (a) mx_adamw_step                                  the un-clipped step
  (b) mx_grad_sumsq + mx_adamw_step_clip             FlatAdamW.step() with a norm clip (the sum of squares is two launches)
  (c) mx_grad_sumsq alone                            4 B read per parameter: the achieved bytes per second are reported
  (d) mx_adamw_step_clip, value mode                 one launch
  (e) mx_reduce_rows_adamw_step                      the fused step_from_rows of the TBPTT loop, clip off
  (f) mx_reduce_rows + (b)                           step_from_rows with a norm clip

as the median, minimum and maximum over `--rounds` rounds of `--reps` back-to-back launches, the forms alternating within a
round.  200 launches of a few microseconds are back-to-back launch throughput on an otherwise idle stream, not a kernel's
latency; a 5 MB gradient also stays in the 256 MiB last-level cache between launches, so the byte rate of (c) is NOT an HBM
figure.  Nothing is gated; this tool is how the numbers in profiles/r13/ are produced.

With `--parent-tree DIR` (a built checkout of the parent commit) it then runs `bench.py --gpus 1 --steps 20 --warmup 5` in
fresh child processes, this tree and the parent's alternating `--bench-rounds` times: with the clip off the optimizer launches
are the parent's, so the two headline figures must agree within the spread of that alternation.

    python tools/clip_step_time.py [--rounds 5] [--reps 200] [--rows 7] [--parent-tree DIR] [--bench-rounds 3] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    """event ms per call of `reps` back-to-back calls, the device drained before and after"""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def time_size(n, rows, rounds, reps, dev):
    from mod_extraction_amd import _hip, optim
    torch.manual_seed(n)
    part = torch.randn(rows, n, device=dev)

    def make(**kw):
        o = optim.FlatAdamW([torch.nn.Parameter(torch.randn(n, device=dev))], lr=1e-4, betas=(0.8, 0.99), **kw)
        o.flat_grad.copy_(torch.randn(n, device=dev))
        return o
    plain, norm, value = make(), make(clip_val=1.0), make(clip_val=0.01, clip_algorithm="value")

    def sumsq():
        _hip.call("mx_grad_sumsq", _hip.ptr(norm.flat_grad), n, _hip.ptr(norm._clip_part), _hip.ptr(norm._clip_stat), _hip.stream())

    work = {"adamw_step": plain.step, "sumsq_plus_adamw_step_clip_norm": norm.step, "grad_sumsq": sumsq,
            "adamw_step_clip_value": value.step, "reduce_rows_adamw_step": lambda: plain.step_from_rows(part),
            "reduce_rows_plus_sumsq_plus_adamw_step_clip": lambda: norm.step_from_rows(part)}
    for fn in work.values():                                    # warm-up: code objects, allocator
        fn()
        fn()
    res = {k: [] for k in work}
    for _ in range(rounds):
        for k, fn in work.items():
            res[k].append(timed(fn, reps))
    out = {k: summary(v) for k, v in res.items()}
    out["grad_sumsq_GB_per_s"] = 4.0 * n / (out["grad_sumsq"]["median"] * 1e-3) / 1e9
    out["clip_norm_over_plain"] = out["sumsq_plus_adamw_step_clip_norm"]["median"] / out["adamw_step"]["median"]
    out["clip_value_over_plain"] = out["adamw_step_clip_value"]["median"] / out["adamw_step"]["median"]
    out["rows_clip_over_fused"] = out["reduce_rows_plus_sumsq_plus_adamw_step_clip"]["median"] / out["reduce_rows_adamw_step"]["median"]
    return out


def bench_line(tree, timeout):
    res = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=tree,
                         capture_output=True, text=True, timeout=timeout)
    if res.returncode != 0:
        raise RuntimeError(f"bench.py in {tree} exited with {res.returncode}: {res.stderr[-1000:]}")
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rows", type=int, default=7, help="gradient rows (clips) of the step_from_rows forms")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    dev = torch.device("cuda:0")
    report = {"rounds": args.rounds, "reps": args.reps, "rows": args.rows, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for n in (1340353, 17473):
        r = time_size(n, args.rows, args.rounds, args.reps, dev)
        report["sizes"][str(n)] = r
        print(f"n = {n}")
        for k, v in r.items():
            if isinstance(v, dict):
                print(f"  {k:46s} {v['median'] * 1e3:9.2f} us [{v['min'] * 1e3:.2f} .. {v['max'] * 1e3:.2f}]")
            else:
                print(f"  {k:46s} {v:9.3f}")
    if args.parent_tree:
        runs = {"this": [], "parent": []}
        for _ in range(args.bench_rounds):
            for name, tree in (("this", ROOT), ("parent", os.path.abspath(args.parent_tree))):
                line = bench_line(tree, args.bench_timeout)
                runs[name].append({"value": line["value"], "ms_per_step": line["ms_per_step"]})
                print(f"bench {name:6s} {line['value']:.1f} {line.get('unit', '')}  ({line['ms_per_step']:.3f} ms / step)", flush=True)
        report["bench"] = {k: {"runs": v, "value": summary([r["value"] for r in v])} for k, v in runs.items()}
    print(json.dumps(report))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()

"""Timing of the FIR match (mod_extraction_amd/fir_match.py, csrc/fir_match.hip, K21) with HIP events and the wall clock,
fixed seed.  It claims nothing until it has run: no figure of this tool is on record unless profiles/ holds its JSON.

  rows     96 x 88200 (a training batch of 2 s clips at 44.1 kHz) and 8 x 22272 (the tests' size): y_hat a noise-driven comb,
           y = y_hat through [0.2, 0.6, 0.15] plus 1 % noise, dz white noise;  K = 9 and K = 32, centred
  cases    fwd        the forward triple of launches (partials, solve, apply) into a preallocated z
           bwd        the backward triple (bwd_partials, bwd_solve, bwd_apply) into a preallocated dy_hat
           torch_fwd  the same function as torch expressions in the same process: an unfold of the padded rows, two einsums
                      for R and b, torch.linalg.solve, a grouped conv1d -- fp32 throughout
           torch_bwd  torch autograd of that expression (the forward graph is built outside the timed call)
           The torch route is the YARDSTICK: fp32, no fp64 sums, no fixed order, no guards.  Where torch.linalg.solve is not
           available on the device the two torch cases are recorded as unavailable with the error's text.
  step     lightning.LFOExtractionThroughEffect on 96 flanger clips of 2 s from the batcher ({"mrstft": 1}, the LFO off the
           label, forward and backward of audio_loss) with match_fir = None, 9 and 32
  times    --rounds rounds of --reps calls, the cases alternating within a round: per call the HIP-event time and the
           wall-clock time (calls enqueued back to back, one synchronisation a round); the median round is reported with
           every round's value

The measurement runs in a child process under a time limit.

    python tools/fir_match_time.py [--reps 20] [--rounds 5] [--out profiles/r22/fir_match_time.json]
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
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT = 400                                                                   # seconds, for the child
SHAPES = ((96, 88200), (8, 22272))
TAPS = (9, 32)
RIDGE, EPS, MAX_GAIN = 1e-6, 1e-8, 20.0


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


def torch_fwd(x, y, K, c):
    B, N = x.shape
    U = F.pad(x, (K - 1, K - 1)).unfold(1, N, 1)                              # U[b, i, n] = x[b, n + i - (K - 1)]
    R = torch.einsum("bkn,bn->bk", U[:, K - 1:], x)
    b = torch.einsum("bkn,bn->bk", U[:, c:c + K].flip(1), y)
    idx = (torch.arange(K, device=x.device)[:, None] - torch.arange(K, device=x.device)[None, :]).abs()
    A = R[:, idx] + (EPS + RIDGE * R[:, :1, None]) * torch.eye(K, device=x.device)
    h = torch.linalg.solve(A, b)
    z = F.conv1d(F.pad(x, (K - 1 - c, c))[None], h.flip(1)[:, None], groups=B)[0]
    return z, h


def measure(args):
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    from mod_extraction_amd import data_modules, fir_match as FM, lightning
    dev = torch.device("cuda:0")
    cases, notes = {}, {}
    for B, N in SHAPES:
        gen = torch.Generator().manual_seed(B)
        v = torch.randn(B, N + 8, generator=gen)
        p = (0.25 * (v[:, 8:] + 0.5 * v[:, 1:N + 1])).contiguous()
        q = 0.2 * p + 0.0025 * torch.randn(B, N, generator=gen)
        q[:, 1:] += 0.6 * p[:, :-1]
        q[:, 2:] += 0.15 * p[:, :-2]
        p, q, dz = p.to(dev), q.to(dev), torch.randn(B, N, generator=gen).to(dev)
        for K in TAPS:
            c = (K - 1) // 2
            z, dy = torch.empty_like(p), torch.empty_like(p)
            m = FM.match_fir(p, q, K, c, RIDGE, EPS, MAX_GAIN, out=z)
            d = FM.match_fir_backward(dz, p, q, m, RIDGE, EPS, c, out=dy)
            assert int(m.flags.sum()) == 0
            tag = f"B{B}_N{N}_K{K}"
            info = {"rows": B, "samples": N, "taps": K}
            cases[f"{tag}_fwd"] = (lambda p=p, q=q, z=z, K=K, c=c: FM.match_fir(p, q, K, c, RIDGE, EPS, MAX_GAIN, out=z),
                                   dict(info, bytes=4 * 4 * B * N))             # y_hat twice, y, z
            cases[f"{tag}_bwd"] = (lambda dz=dz, p=p, q=q, m=m, dy=dy, c=c: FM.match_fir_backward(dz, p, q, m, RIDGE, EPS, c, out=dy),
                                   dict(info, bytes=6 * 4 * B * N))             # dz and y_hat twice, y, dy_hat
            try:
                pg = p.clone().requires_grad_(True)
                zt, ht = torch_fwd(pg, q, K, c)
                dt, = torch.autograd.grad(zt, pg, dz, retain_graph=True)
                torch.cuda.synchronize()
                info_t = dict(info, fwd_max_rel_diff_to_torch=float(((z - zt.detach()).abs().max() / zt.detach().abs().max()).cpu()),
                              bwd_max_rel_diff_to_torch=float(((d - dt).abs().max() / dt.abs().max()).cpu()))
                cases[f"{tag}_torch_fwd"] = (lambda p=p, q=q, K=K, c=c: torch_fwd(p, q, K, c), info_t)
                cases[f"{tag}_torch_bwd"] = (lambda zt=zt, pg=pg, dz=dz: torch.autograd.grad(zt, pg, dz, retain_graph=True), info_t)
            except Exception as e:                                            # no solver library on the device, or no memory
                notes[f"{tag}_torch"] = f"unavailable: {type(e).__name__}: {str(e)[:200]}"
    # the step: 96 flanger clips of 2 s
    Bs, Ns = 96, 88200
    torch.manual_seed(7)
    np.random.seed(7)
    batcher = data_modules.SyntheticFxBatcher(Bs, Ns, 44100, ("flanger",), dev, audio_seed=7, fixed_lead=0)
    dry, wet, mod, fxp = batcher.render(batcher.sample_params())
    t = torch.linspace(0.0, 1.0, mod.size(1), device=dev)
    h0 = (mod + 0.1 * torch.sin(2 * math.pi * 1.5 * t)[None, :]).clamp(0.0, 1.0).contiguous()
    for K in (None,) + TAPS:
        step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=44100, effect="flanger",
                                                    audio_loss_dict={"mrstft": 1.0}, match_fir=K).to(dev)

        def run(step=step):
            h = h0.clone().requires_grad_(True)
            loss, _ = step.audio_loss(h, dry, wet, fxp)
            loss.backward()

        cases[f"step_B{Bs}_N{Ns}_match_fir_{K}"] = (run, {"rows": Bs, "samples": Ns, "taps": K})
    for fn, _ in cases.values():
        fn()
    torch.cuda.synchronize()
    ev, wall = {k: [] for k in cases}, {k: [] for k in cases}
    for _ in range(args.rounds):
        for k, (fn, _) in cases.items():
            e, w = timed(fn, max(1, args.reps // 4) if k.startswith("step_") else args.reps)
            ev[k].append(e)
            wall[k].append(w)
    out = {"device": torch.cuda.get_device_name(0), "cases": {}, "faster_than_torch": {}, "notes": notes}
    for k, (_, info) in cases.items():
        med = float(np.median(ev[k]))
        row = dict(info, event_median_ms=med, wall_median_ms=float(np.median(wall[k])),
                   event_rounds_ms=[round(x, 4) for x in ev[k]], wall_rounds_ms=[round(x, 4) for x in wall[k]])
        if "bytes" in info:
            row["gbytes_per_s"] = info["bytes"] / (med * 1e-3) / 1e9
        out["cases"][k] = row
        print(f"  {k:34s} events {med:9.4f} ms   wall {row['wall_median_ms']:9.4f} ms   (event rounds: {row['event_rounds_ms']})")
    for k, v in notes.items():
        print(f"  {k}: {v}")
    for B, N in SHAPES:
        for K in TAPS:
            for way in ("fwd", "bwd"):
                mine, ref = out["cases"].get(f"B{B}_N{N}_K{K}_{way}"), out["cases"].get(f"B{B}_N{N}_K{K}_torch_{way}")
                if ref is None:
                    continue
                verdict = {"events": mine["event_median_ms"] < ref["event_median_ms"], "wall": mine["wall_median_ms"] < ref["wall_median_ms"]}
                out["faster_than_torch"][f"B{B}_N{N}_K{K}_{way}"] = verdict
                print(f"  B{B}_N{N}_K{K}_{way}: the three launches are {'FASTER' if verdict['events'] else 'NOT faster'} than the torch "
                      f"route by events, {'FASTER' if verdict['wall'] else 'NOT faster'} by the wall clock")
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

"""Timing of the shaper match (mod_extraction_amd/shaper.py, csrc/shaper_match.hip, K27) with HIP events and the wall clock,
fixed seed.  It claims nothing until it has run: no figure of this tool is on record unless profiles/ holds its JSON.

  rows     8 x 22272 (the tests' size) and 96 x 88200 (a training batch of 2 s clips at 44.1 kHz): y_hat a noise-driven comb at
           peak 0.25, y = 0.25 pk tanh(2 y_hat / pk), dz white noise;  orders 3 and 7, odd powers
  cases    fwd        the forward triple of calls (partials, solve, apply) into a preallocated z
           bwd        the backward triple (bwd_partials, bwd_solve, bwd_apply) into a preallocated dy_hat
           torch_fwd  the same function as torch expressions in the same process: the basis t^p stacked, two batched products
                      for A and b, torch.linalg.solve, one more product -- in fp64, since an fp32 Gram matrix of monomials up
                      to t^14 (cond ~ 1e6) holds no digits
           torch_bwd  torch autograd of that expression (the forward graph is built outside the timed call)
           The torch route is the YARDSTICK: no fixed order, no guards, K rows of N doubles of workspace.  Where
           torch.linalg.solve is not available on the device the two torch cases are recorded as unavailable with the error.
  step     lightning.LFOExtractionThroughEffect on 96 flanger clips of 2 s from the batcher ({"mrstft": 1}, the LFO off the
           label, forward and backward of audio_loss) with match_shaper = None and 5.  Without the key the step makes the
           parent's calls with the parent's arguments (tests/test_gpu_shaper_step.py), so the two alternate in one process.
  times    --rounds rounds of --reps calls, the cases alternating within a round: per call the HIP-event time and the
           wall-clock time (calls enqueued back to back, one synchronisation a round); the median round is reported with
           every round's value

The measurement runs in a child process under a time limit.

    python tools/shaper_match_time.py [--reps 20] [--rounds 5] [--out profiles/r29/shaper_match_time.json]
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT = 400                                                                   # seconds, for the child
SHAPES = ((8, 22272), (96, 88200))
ORDERS = (3, 7)
RIDGE, MAX_GAIN = 1e-9, 20.0


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


def torch_fwd(x, y, powers):
    x64, y64 = x.double(), y.double()
    r = x64.pow(2).mean(1, keepdim=True).sqrt()
    t = x64 / r
    basis = torch.stack([t ** p for p in powers], 1)                          # (B, K, N)
    A = basis @ basis.transpose(1, 2)
    A = A + RIDGE * torch.diag_embed(torch.diagonal(A, dim1=1, dim2=2))
    c = torch.linalg.solve(A, basis @ (y64 / r).unsqueeze(2))                 # (B, K, 1)
    return (r * (c.transpose(1, 2) @ basis)[:, 0]).float()


def measure(args):
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    from mod_extraction_amd import data_modules, lightning, shaper as SH
    dev = torch.device("cuda:0")
    cases, notes = {}, {}
    for B, N in SHAPES:
        gen = torch.Generator().manual_seed(B)
        v = torch.randn(B, N + 37, generator=gen)
        p = v[:, 37:] + 0.7 * v[:, :N]
        pk = p.abs().amax(1, keepdim=True)
        p = (0.25 * p / pk).contiguous()
        q = 0.25 * 0.25 * torch.tanh(2.0 * p / 0.25)
        p, q, dz = p.to(dev), q.to(dev), torch.randn(B, N, generator=gen).to(dev)
        for order in ORDERS:
            z, dy = torch.empty_like(p), torch.empty_like(p)
            m = SH.match_shaper(p, q, order, False, RIDGE, MAX_GAIN, out=z)
            d = SH.match_shaper_backward(dz, p, q, m, False, RIDGE, out=dy)
            assert int(m.flags.sum()) == 0
            tag = f"B{B}_N{N}_P{order}"
            info = {"rows": B, "samples": N, "order": order}
            cases[f"{tag}_fwd"] = (lambda p=p, q=q, z=z, order=order: SH.match_shaper(p, q, order, False, RIDGE, MAX_GAIN, out=z),
                                   dict(info, bytes=5 * 4 * B * N))             # y_hat three times, y, z
            cases[f"{tag}_bwd"] = (lambda dz=dz, p=p, q=q, m=m, dy=dy: SH.match_shaper_backward(dz, p, q, m, False, RIDGE, out=dy),
                                   dict(info, bytes=6 * 4 * B * N))             # dz and y_hat twice, y, dy_hat
            try:
                pg = p.clone().requires_grad_(True)
                zt = torch_fwd(pg, q, SH.powers(order))
                dt, = torch.autograd.grad(zt, pg, dz, retain_graph=True)
                torch.cuda.synchronize()
                info_t = dict(info, fwd_max_rel_diff_to_torch=float(((z - zt.detach()).abs().max() / zt.detach().abs().max()).cpu()),
                              bwd_max_rel_diff_to_torch=float(((d - dt).abs().max() / dt.abs().max()).cpu()))
                cases[f"{tag}_torch_fwd"] = (lambda p=p, q=q, order=order: torch_fwd(p, q, SH.powers(order)), info_t)
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
    for order in (None, 5):
        step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=44100, effect="flanger",
                                                    audio_loss_dict={"mrstft": 1.0}, match_shaper=order).to(dev)

        def run(step=step):
            h = h0.clone().requires_grad_(True)
            loss, _ = step.audio_loss(h, dry, wet, fxp)
            loss.backward()

        cases[f"step_B{Bs}_N{Ns}_match_shaper_{order}"] = (run, {"rows": Bs, "samples": Ns, "order": order})
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
        print(f"  {k:38s} events {med:9.4f} ms   wall {row['wall_median_ms']:9.4f} ms   (event rounds: {row['event_rounds_ms']})")
    for k, v in notes.items():
        print(f"  {k}: {v}")
    for B, N in SHAPES:
        for order in ORDERS:
            for way in ("fwd", "bwd"):
                mine, ref = out["cases"].get(f"B{B}_N{N}_P{order}_{way}"), out["cases"].get(f"B{B}_N{N}_P{order}_torch_{way}")
                if ref is None:
                    continue
                verdict = {"events": mine["event_median_ms"] < ref["event_median_ms"], "wall": mine["wall_median_ms"] < ref["wall_median_ms"]}
                out["faster_than_torch"][f"B{B}_N{N}_P{order}_{way}"] = verdict
                print(f"  B{B}_N{N}_P{order}_{way}: the three calls are {'FASTER' if verdict['events'] else 'NOT faster'} than the torch "
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

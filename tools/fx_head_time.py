"""Timing of the per-clip effect-parameter head (fx.FxParamHead, csrc/fx_head.hip) with HIP events, fixed seed.  It claims
nothing until it has run: no figure of this tool is on record unless profiles/ holds its JSON.

  head_fwd / head_bwd   the two entry points alone at B = 64 and 256 clips, C = 64 channels, W = 345 frames (the shipped
                        model's latent: 88 KB per clip, read once by the forward, written once by the backward's d_latent),
                        the table of configs/train_lfo_pairs_flanger_head.yml (P = 2); --rounds rounds of --reps launches,
                        the two alternating within a round; with them the bytes of the latent over the time, as a figure to
                        compare the two by, not a roofline claim
  step_batch            the single-effect flanger step, --batch clips (default 96) of 2 s, fx_params from the batch
  step_learned          the same step with the learned_fx of configs/train_lfo_pairs_flanger.yml
  step_head             the same step with the fx_head of configs/train_lfo_pairs_flanger_head.yml and a (B, 64, 345) latent
                        that requires grad (so the d_latent write is part of it)
                        -- the three steps alternating, --step-reps launches a round

The median round is reported with every round's value.  The measurement runs in a child process under a time limit.

    python tools/fx_head_time.py [--batch 96] [--reps 200] [--step-reps 5] [--rounds 5] [--out profiles/r17/fx_head_time.json]
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
SR = 44100
LIMIT = 300                                                                   # seconds, for the child
FIXED = {"width": 1.0, "min_delay_width": 0.5}
LEARNED = {"flanger": dict(FIXED, feedback={"min": 0.0, "max": 0.95, "init": 0.3}, depth={"min": 0.0, "max": 1.0, "init": 0.5},
                           mix={"min": 0.0, "max": 1.0, "init": 0.5})}
HEAD = {"flanger": dict(FIXED, feedback={"min": 0.0, "max": 0.95, "init": 0.3}, depth={"min": 0.0, "max": 1.0, "init": 0.5},
                        mix=1.0)}


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternate(fns, reps, rounds):
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            t[k].append(timed(f, reps))
    return {k: {"median_ms": float(np.median(v)), "rounds_ms": [round(x, 5) for x in v]} for k, v in t.items()}


def kernels(B, reps, rounds, dev):
    from mod_extraction_amd import fx
    C, W = 64, 345
    head = fx.FxParamHead(HEAD, in_ch=C).to(dev)
    g = torch.Generator().manual_seed(B)
    with torch.no_grad():
        head.weight.copy_(0.1 * torch.randn(head.weight.shape, generator=g))
    latent = torch.randn(B, C, W, generator=g).to(dev)
    row_kind = torch.zeros(B, dtype=torch.int32, device=dev)
    ml, mm = torch.full((B,), 441.0, device=dev), torch.full((B,), 44.0, device=dev)
    consts = {k: torch.zeros(B, device=dev) for k in ("feedback", "depth")}
    pooled, raw_rows, _ = head.forward_rows(latent, consts, row_kind, ml, mm)
    grads = torch.randn(6, B, generator=g, dtype=torch.float64).to(dev)
    fns = {"head_fwd": lambda: head.forward_rows(latent, consts, row_kind, ml, mm),
           "head_bwd": lambda: head.backward_rows(grads, raw_rows, pooled, row_kind, ml, mm, W)}
    res = alternate(fns, reps, rounds)
    nbytes = latent.numel() * 4
    for k, v in res.items():
        v["latent_gb_per_s"] = nbytes / (v["median_ms"] * 1e-3) / 1e9
        print(f"  B {B:4d} {k:9s} {v['median_ms'] * 1e3:8.2f} us   latent bytes / time {v['latent_gb_per_s']:8.1f} GB/s   "
              f"(rounds, ms: {v['rounds_ms']})")
    return dict(res, clips=B, channels=C, frames=W, latent_bytes=nbytes)


def steps(B, reps, rounds, dev):
    from mod_extraction_amd import data_modules, lightning
    from mod_extraction_amd.util import linear_interpolate_last_dim
    N = 2 * SR
    torch.manual_seed(0)
    np.random.seed(0)
    bt = data_modules.SyntheticFxBatcher(B, N, SR, ("flanger",), dev, audio_seed=0, overlap=False)
    dry, wet, mod, fxp = bt.next_batch()
    lfo = linear_interpolate_last_dim(mod, N // 256 + 1, align_corners=True).contiguous()
    ident, losses = torch.nn.Identity(), {"mrstft": 1.0}
    plain = lightning.LFOExtractionThroughEffect(ident, sr=SR, effect="flanger", audio_loss_dict=losses)
    learned = lightning.LFOExtractionThroughEffect(ident, sr=SR, effect="flanger", audio_loss_dict=losses,
                                                   learned_fx=LEARNED).to(dev)
    headed = lightning.LFOExtractionThroughEffect(ident, sr=SR, effect="flanger", audio_loss_dict=losses, fx_head=HEAD).to(dev)
    with torch.no_grad():
        headed.fx_head.weight.normal_(0.0, 0.05)
    latent = torch.randn(B, 64, lfo.size(1), device=dev)

    def step_fn(step, fx_params, params, with_latent):
        h = lfo.clone().requires_grad_(True)
        z = latent.clone().requires_grad_(True) if with_latent else None

        def run():
            for p in [h, z] + params:
                if p is not None:
                    p.grad = None
            step.audio_loss(h, dry, wet, fx_params, latent=z)[0].backward()
        return run

    fns = {"step_batch": step_fn(plain, fxp, [], False),
           "step_learned": step_fn(learned, None, [learned.learned_fx.raw], False),
           "step_head": step_fn(headed, None, list(headed.fx_head.parameters()), True)}
    res = alternate(fns, reps, rounds)
    print(f"flanger draw: {B} clips x {N} samples, LFO and latent {lfo.size(1)} frames")
    for k, v in res.items():
        print(f"  {k:13s} {v['median_ms']:.4f} ms   (rounds: {v['rounds_ms']})")
    return dict(res, clips=B, samples=N, frames=lfo.size(1))


def measure(args):
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "kernels": [kernels(B, args.reps, args.rounds, dev) for B in (64, 256)],
           "flanger_step": steps(args.batch, args.step_reps, args.rounds, dev)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=96)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step-reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the results as JSON")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(measure(args)))
        return 0
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child", "--batch", str(args.batch),
           "--reps", str(args.reps), "--step-reps", str(args.step_reps), "--rounds", str(args.rounds)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    lines = p.stdout.splitlines()
    print("\n".join(l for l in lines if not l.startswith("RESULT ")), flush=True)
    if p.returncode != 0:
        print(f"exit status {p.returncode}")
        return p.returncode
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(json.loads(next(l for l in lines if l.startswith("RESULT "))[7:]), reps=args.reps,
                           step_reps=args.step_reps, rounds=args.rounds), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Timing of the audio-loss step with learned effect parameters (lightning.LFOExtractionThroughEffect(learned_fx=...),
csrc/fx_params.hip) beside the step that reads them from the batch, with HIP events, fixed seed.  It claims nothing until
it has run: no figure of this tool is on record unless profiles/ holds its JSON.

Shape: the single-effect flanger step on the batcher's draw, --batch clips (default 96) of 2 s, the label resampled to the
extractor's frame rate (345 points), audio_loss_dict {mrstft: 1.0}.

  step_batch    fx_params from the batch: the path of a tree without learned_fx (run this tool there too: it then
                measures this entry alone)
  step_learned  the same step with the learned_fx of configs/train_lfo_pairs_flanger.yml (feedback, depth, mix learned, the
                two widths fixed) on a (dry, wet, None, None) batch: mx_fx_params_expand, the adjoint asked for three
                per-clip gradients, mx_fx_params_grad
  expand / grad the two new launches alone

The entries are timed alternately, --rounds times --reps launches each; the median round is reported with every round's
value.  The measurement runs in a child process under a time limit.

    python tools/fx_params_step_time.py [--batch 96] [--reps 5] [--rounds 5] [--out profiles/r16/fx_params_step_time.json]
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
LEARNED = {"flanger": {"feedback": {"min": 0.0, "max": 0.95, "init": 0.3}, "depth": {"min": 0.0, "max": 1.0, "init": 0.5},
                       "mix": {"min": 0.0, "max": 1.0, "init": 0.5}, "width": 1.0, "min_delay_width": 0.5}}


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
    return {k: {"median_ms": float(np.median(v)), "rounds_ms": [round(x, 4) for x in v]} for k, v in t.items()}


def step_fn(step, dry, wet, fxp, lfo, raw=None):
    h = lfo.clone().requires_grad_(True)

    def run():
        h.grad = None
        if raw is not None:
            raw.grad = None
        step.audio_loss(h, dry, wet, fxp)[0].backward()
    return run


def measure(B, reps, rounds):
    from mod_extraction_amd import data_modules, fx, lightning
    from mod_extraction_amd.util import linear_interpolate_last_dim
    dev = torch.device("cuda:0")
    N = 2 * SR
    torch.manual_seed(0)
    np.random.seed(0)
    bt = data_modules.SyntheticFxBatcher(B, N, SR, ("flanger",), dev, audio_seed=0, overlap=False)
    dry, wet, mod, fxp = bt.next_batch()
    lfo = linear_interpolate_last_dim(mod, N // 256 + 1, align_corners=True).contiguous()
    ident, losses = torch.nn.Identity(), {"mrstft": 1.0}
    plain = lightning.LFOExtractionThroughEffect(ident, sr=SR, effect="flanger", audio_loss_dict=losses)
    fns = {"step_batch": step_fn(plain, dry, wet, fxp, lfo)}
    has = hasattr(fx, "LearnedFxParams")
    if has:
        step = lightning.LFOExtractionThroughEffect(ident, sr=SR, effect="flanger", audio_loss_dict=losses,
                                                    learned_fx=LEARNED).to(dev)
        lf = step.learned_fx
        fns["step_learned"] = step_fn(step, dry, wet, None, lfo, lf.raw)
        m = step._mixed_rows(B, dev)
        consts = step.clip_constants(None, B, dev)
        gbuf = torch.randn(6, B, device=dev, dtype=torch.float64)
        fns["expand"] = lambda: lf.expand(consts, m["row_kind"], m["max_lfo_delay"], m["max_min_delay"])
        fns["grad"] = lambda: lf.grad(gbuf, m["row_kind"], m["max_lfo_delay"], m["max_min_delay"])
    res = alternate(fns, reps, rounds)
    print(f"flanger draw: {B} clips x {N} samples, LFO {lfo.size(1)} points, learned_fx {'present' if has else 'ABSENT in this tree'}")
    for k, v in res.items():
        print(f"  {k:13s} {v['median_ms']:.4f} ms   (rounds: {v['rounds_ms']})")
    return dict(res, clips=B, samples=N, lfo_points=lfo.size(1), learned_fx=has)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=96)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the results as JSON")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(measure(args.batch, args.reps, args.rounds)))
        return 0
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child", "--batch", str(args.batch),
           "--reps", str(args.reps), "--rounds", str(args.rounds)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    lines = p.stdout.splitlines()
    print("\n".join(l for l in lines if not l.startswith("RESULT ")), flush=True)
    if p.returncode != 0:
        print(f"exit status {p.returncode}")
        return p.returncode
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"reps": args.reps, "rounds": args.rounds, "flanger": json.loads(
                next(l for l in lines if l.startswith("RESULT "))[7:])}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

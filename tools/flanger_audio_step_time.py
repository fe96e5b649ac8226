"""Timing of the flanger adjoint for a low-rate LFO and of the training step built on it, with HIP events, fixed seed.

Shapes: config 5's (256 flanger clips x 4 s) and config 3's flanger / chorus draw (the 171 effect rows of 256 interwoven
clips x 2 s, both geometries in one launch).  The LFO is the batch's label resampled to the extractor's frame rate
(N // 256 + 1 points: 690 resp. 345).

  (a) low rate     mx_flanger_fwd_stash on the (B, n_frames) row + mx_flanger_bwd_lr (dmod (B, n_frames))
  (b) full rate    the route without the low-rate adjoint: linear_interpolate_last_dim to (B, N), mx_flanger_fwd_stash,
                   mx_flanger_bwd (dmod (B, N)), linear_interpolate_last_dim_bwd
  (c) step         LFOExtractionThroughEffect on 256 flanger clips: audio_loss forward + backward for a free LFO at config
                   5's shape (stash forward, MR-STFT value and gradient, low-rate backward: everything the step adds to the
                   extractor), and the whole training_step with the shipped Spectral2DCNN on 2 s clips (forward + backward,
                   no optimizer).  The step takes one geometry per module, so config 3's mixed draw has no (c).

(a) and (b) are timed alternately, --rounds times --reps launches each; the median round is reported with every round's
value.  Each case runs in a child process of its own under a time limit; the first failure ends the run.

    python tools/flanger_audio_step_time.py [--reps 10] [--rounds 5] [--out profiles/r08/flanger_audio_step_time.json]
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
CASES = {"config5": 300, "config3": 300, "step_config5": 300, "step_cnn_2s": 600}        # name -> time limit, seconds


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


def draw(batch, seconds, kinds, dev, seed):
    """The flanger / chorus rows of one batch of the synthetic batcher, dense, with their per-clip constants."""
    from mod_extraction_amd import data_modules
    from mod_extraction_amd.util import linear_interpolate_last_dim
    N = int(seconds * SR)
    torch.manual_seed(seed)
    np.random.seed(seed)
    bt = data_modules.SyntheticFxBatcher(batch, N, SR, kinds, dev, audio_seed=seed, overlap=False)
    dry, wet, mod, d = bt.next_batch()
    idx = bt.rows_fx.long()
    consts = {"lfo_scale": d["width"] * bt.max_lfo_delay, "min_delay": d["min_delay_width"] * bt.max_min_delay,
              "feedback": d["feedback"], "depth": d["depth"], "mix": d["mix"], "one_minus_mix": 1.0 - d["mix"]}
    consts = {k: v[idx].float().contiguous() for k, v in consts.items()}
    lfo = linear_interpolate_last_dim(mod[idx].contiguous(), N // 256 + 1, align_corners=True).contiguous()
    return (dry[idx, 0].contiguous(), wet[idx, 0].contiguous(), lfo, consts, bt.max_delay[idx].contiguous(),
            bt.max_delay_max, {k: v[idx] for k, v in d.items() if isinstance(v, torch.Tensor)})


def adjoint_case(name, batch, seconds, kinds, reps, rounds):
    from mod_extraction_amd import fx
    from mod_extraction_amd.util import linear_interpolate_last_dim, linear_interpolate_last_dim_bwd
    dev = torch.device("cuda:0")
    x, _, lfo, consts, md, M, _ = draw(batch, seconds, kinds, dev, 0)
    B, N = x.shape
    n_f = lfo.size(1)
    dy = torch.randn(B, N, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    y, st = torch.empty_like(x), torch.empty_like(x)
    dm_lr, dm_full = torch.empty_like(lfo), torch.empty_like(x)

    def low():
        fx.flanger_forward_stash(x, lfo, consts, md, M, out=y, stash=st)
        fx.flanger_backward(dy, x, lfo, st, consts, md, M, need_dx=False, params=(), dmod=dm_lr)

    def full():
        up = linear_interpolate_last_dim(lfo, N, align_corners=True)
        fx.flanger_forward_stash(x, up, consts, md, M, out=y, stash=st)
        fx.flanger_backward(dy, x, up, st, consts, md, M, need_dx=False, params=(), dmod=dm_full)
        return linear_interpolate_last_dim_bwd(dm_full, n_f, N)

    res = alternate({"a_low_rate": low, "b_full_rate": full}, reps, rounds)
    a, b = res["a_low_rate"]["median_ms"], res["b_full_rate"]["median_ms"]
    print(f"{name}: {B} clips x {N} samples, LFO {n_f} points")
    print(f"  (a) low rate   {a:.3f} ms   (rounds: {res['a_low_rate']['rounds_ms']})")
    print(f"  (b) full rate  {b:.3f} ms   (rounds: {res['b_full_rate']['rounds_ms']})   (a) / (b) = {a / b:.3f}")
    return dict(res, clips=B, samples=N, lfo_points=n_f, a_over_b=round(a / b, 4))


def step_case(name, seconds, with_cnn, reps, rounds):
    from mod_extraction_amd import data_modules, lightning, models
    dev = torch.device("cuda:0")
    B, N = 256, int(seconds * SR)
    torch.manual_seed(0)
    np.random.seed(0)
    bt = data_modules.SyntheticFxBatcher(B, N, SR, ("flanger",), dev, audio_seed=0, overlap=False)
    dry, wet, mod, fxp = bt.next_batch()
    if with_cnn:
        cnn = models.Spectral2DCNN(in_ch=2, n_samples=N, sr=SR, n_fft=1024, hop_len=256, n_mels=256, kernel_size=(5, 13),
                                   out_channels=[64] * 6, temp_dilations=[1, 1, 2, 4, 8, 16], pool_size=(2, 1), latent_dim=1,
                                   freq_mask_amount=0.25, time_mask_amount=0.25, use_ln=True)
        step = lightning.LFOExtractionThroughEffect(cnn, sr=SR, audio_loss_dict={"mrstft": 1.0}).to(dev).train()

        def run():
            step.zero_grad()
            step.training_step((dry, wet, None, fxp)).backward()
            step.logged.clear()
    else:
        from mod_extraction_amd.util import linear_interpolate_last_dim
        step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, audio_loss_dict={"mrstft": 1.0})
        h = linear_interpolate_last_dim(mod, N // 256 + 1, align_corners=True).contiguous().requires_grad_(True)

        def run():
            h.grad = None
            step.audio_loss(h, dry, wet, fxp)[0].backward()

    res = alternate({"c_step": run}, reps, rounds)
    print(f"{name}: {B} flanger clips x {N} samples{', Spectral2DCNN' if with_cnn else ', free LFO'}")
    print(f"  (c) step       {res['c_step']['median_ms']:.3f} ms   (rounds: {res['c_step']['rounds_ms']})")
    return dict(res, clips=B, samples=N)


def run_case(case, reps, rounds):
    if case == "config5":
        return adjoint_case("config 5 shape", 256, 4.0, ("flanger",), reps, rounds)
    if case == "config3":
        return adjoint_case("config 3 flanger / chorus draw", 256, 2.0, ("flanger", "chorus", "phaser"), reps, rounds)
    if case == "step_config5":
        return step_case("config 5 shape", 4.0, False, reps, rounds)
    return step_case("2 s clips", 2.0, True, reps, rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the results as JSON")
    ap.add_argument("--case", choices=list(CASES), default=None, help="(internal) run one case in this process")
    args = ap.parse_args()
    if args.case:
        print("RESULT " + json.dumps(run_case(args.case, args.reps, args.rounds)))
        return 0
    results = {}
    for case, limit in CASES.items():          # a fresh child per case, each under its own time limit; stop at the first failure
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--case", case,
               "--reps", str(args.reps), "--rounds", str(args.rounds)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = p.stdout.splitlines()
        print("\n".join(l for l in lines if not l.startswith("RESULT ")), flush=True)
        if p.returncode != 0:
            print(f"{case}: exit status {p.returncode}; nothing further is started")
            return p.returncode
        results[case] = json.loads(next(l for l in lines if l.startswith("RESULT "))[7:])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"reps": args.reps, "rounds": args.rounds, "cases": results}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

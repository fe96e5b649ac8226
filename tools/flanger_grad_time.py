"""Timing of the differentiable flanger (mx_flanger_fwd_stash + mx_flanger_bwd) with HIP events, fixed seed.  Prints:

  (a)-(c) on config 3's flanger / chorus draw (the 171 effect rows of 256 x 2 s, full-rate LFO): mx_flanger_fwd, the stash
          forward and the backward, with the ratios stash / fwd and bwd / fwd, and what bounds the backward: the reverse
          lock-steps of the slowest clip (the forward's dependency-free runs, split where a scatter slot would repeat),
          counted on the host, and the backward's time per lock-step
  (d)     a differentiable config-5 step at 256 x 4 s (batch render, stash forward, MR-STFT value and gradient, flanger
          backward) against bench.py's stand-in step (batch render, MR-STFT on lerp(dry, wet, 0.9), loss.backward())

    python tools/flanger_grad_time.py [--reps 10]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SR = 44100


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def consts_of(bt, d):
    return {"lfo_scale": (d["width"] * bt.max_lfo_delay).contiguous(),
            "min_delay": (d["min_delay_width"] * bt.max_min_delay).contiguous(),
            "feedback": d["feedback"].contiguous(), "depth": d["depth"].contiguous(), "mix": d["mix"].contiguous(),
            "one_minus_mix": (1.0 - d["mix"]).contiguous()}


def reverse_lock_steps(mod, ls, md, M):
    """Lock-steps of mx_flanger_bwd's serial kernel for one clip: per row of 64 samples the forward's maximal
    dependency-free runs, also split where the age of the value read at prev (or next) does not increase."""
    N = mod.size
    d = (np.float32(ls) * mod.astype(np.float32) + np.float32(md)).astype(np.float32)
    n = np.arange(N)
    w = n % M
    r = np.mod((w.astype(np.float32) - d).astype(np.float32) + np.float32(M), np.float32(M)).astype(np.float32)
    prev = np.clip(np.floor(r).astype(np.int64), 0, M - 1)
    nxt = (prev + 1) % M
    dp = w - prev; dp[dp <= 0] += M
    dn = w - nxt; dn[dn <= 0] += M
    dep = np.minimum(dp, dn)
    n_rows = -(-N // 64)
    pad = n_rows * 64 - N
    k = np.arange(64)[None, :]
    dep = np.concatenate([dep, np.full(pad, 1 << 30)]).reshape(n_rows, 64)
    t = np.where(dep > k, -1, k - dep)
    age_p = np.concatenate([n - dp, np.zeros(pad, np.int64)]).reshape(n_rows, 64)
    age_n = np.concatenate([n - dn, np.zeros(pad, np.int64)]).reshape(n_rows, 64)
    split = np.zeros_like(t, bool)
    split[:, 1:] = (age_p[:, 1:] <= age_p[:, :-1]) | (age_n[:, 1:] <= age_n[:, :-1])
    valid = (np.arange(n_rows * 64) < N).reshape(n_rows, 64)
    t = np.where(split & valid, np.maximum(t, k - 1), t)
    a = np.zeros(n_rows, np.int64)
    steps = 0
    while True:
        live = a < 64
        if not live.any():
            break
        steps += int(live.sum())
        conflict = (k >= a[:, None]) & (t >= a[:, None])
        first = np.where(conflict.any(axis=1), conflict.argmax(axis=1), 64)
        a = np.where(live, first, a)
    return steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    from mod_extraction_amd import data_modules, fx, losses, mrstft, util
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    np.random.seed(0)

    N = 2 * SR
    bt = data_modules.SyntheticFxBatcher(256, N, SR, ("flanger", "chorus", "phaser"), dev, audio_seed=0, overlap=False)
    dry, wet, mod, p = bt.next_batch()
    rows = bt.rows_fx
    idx = rows.long()
    x = dry[idx, 0].contiguous()
    mod_full = util.linear_interpolate_last_dim(mod[idx].contiguous(), N).contiguous()
    d = {k: v[idx].contiguous() for k, v in p.items() if isinstance(v, torch.Tensor)}
    sub = type("B", (), {"max_lfo_delay": bt.max_lfo_delay[idx], "max_min_delay": bt.max_min_delay[idx]})
    c = consts_of(sub, d)
    md = bt.max_delay[idx].contiguous()
    y = torch.empty_like(x)
    t_fwd = timed(lambda: fx.flanger_forward(x, mod_full, c, md, bt.max_delay_max, out=y), args.reps)
    y2, st = fx.flanger_forward_stash(x, mod_full, c, md, bt.max_delay_max)
    assert torch.equal(y, y2)
    t_st = timed(lambda: fx.flanger_forward_stash(x, mod_full, c, md, bt.max_delay_max, out=y2, stash=st), args.reps)
    dy = torch.randn_like(x)
    t_bwd = timed(lambda: fx.flanger_backward(dy, x, mod_full, st, c, md, bt.max_delay_max), args.reps)
    mh, ch = mod_full.cpu().numpy(), {k: v.cpu().numpy() for k, v in c.items()}
    Ms = md.cpu().numpy()
    steps = [reverse_lock_steps(mh[i], ch["lfo_scale"][i], ch["min_delay"][i], int(Ms[i])) for i in range(len(Ms))]
    worst = max(steps)
    print(f"(a) config 3 draw ({len(Ms)} flanger/chorus clips x 2 s): mx_flanger_fwd {t_fwd:.3f} ms")
    print(f"(b) stash forward {t_st:.3f} ms = {t_st / t_fwd:.2f}x mx_flanger_fwd")
    print(f"(c) mx_flanger_bwd {t_bwd:.3f} ms = {t_bwd / t_fwd:.2f}x mx_flanger_fwd; slowest clip {worst} reverse lock-steps "
          f"(mean {np.mean(steps):.0f}) -> {1e6 * t_bwd / worst:.0f} ns per lock-step")

    N = 4 * SR
    bt = data_modules.SyntheticFxBatcher(256, N, SR, ("flanger",), dev, audio_seed=45, overlap=False)
    loss_fn = losses.get_loss_func_by_name("mrstft")
    mr = mrstft.MultiResolutionSTFTLoss()

    def standin():
        dry, wet, _, _ = bt.next_batch()
        pred = torch.lerp(dry, wet, 0.9).requires_grad_(True)
        loss = loss_fn(pred, wet)
        loss.backward()
        return loss.detach()

    def differentiable():
        dry, wet, mod, p = bt.next_batch()
        mf = util.linear_interpolate_last_dim(mod, N)
        d = {k: v for k, v in p.items() if isinstance(v, torch.Tensor)}
        c = consts_of(bt, d)
        c["feedback"] = (0.9 * c["feedback"]).contiguous()              # a prediction off the target's parameters
        xr = dry[:, 0]
        y, st = fx.flanger_forward_stash(xr, mf, c, bt.max_delay, bt.max_delay_max)
        loss, g = mrstft.mrstft_value_and_grad(mr, y, wet[:, 0])
        fx.flanger_backward(g, xr, mf, st, c, bt.max_delay, bt.max_delay_max)
        return loss

    t_s = timed(standin, args.reps)
    t_d = timed(differentiable, args.reps)
    print(f"(d) config-5 step 256 x 4 s: differentiable {t_d:.2f} ms, stand-in {t_s:.2f} ms = {t_d / t_s:.2f}x")


if __name__ == "__main__":
    main()

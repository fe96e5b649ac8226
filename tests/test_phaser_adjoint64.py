"""CPU: the fp64 phaser adjoint (tests/helpers/phaser_adjoint64.py) against
  (a) oracle.fx.phaser_np: the helper's fp32 forward and its clamped lfo are the oracle's, bit for bit, with the built-in
      oscillator;
  (b) torch autograd in float64 through the recurrence restated in torch (gates 1e-10 of max |g| for dx / dmod and 1e-10
      relative for the parameters, as tests/test_flanger_adjoint64.py);
  (c) central finite differences of the fp64 forward away from the clip edges (1e-6 relative), and the closed forms
      mix = 0 (dx = dy, everything else 0) and depth = 0 (dmod = 0).
Also the convention of the external LFO: see test_mod_is_the_reference_ground_truth_lfo."""
import math

import numpy as np
import torch

from oracle import fx as ofx, modulations as omod
from tests.helpers.phaser_adjoint64 import (PARAMS, builtin_osc, chain32, forward32, forward64, phaser_adjoint64)

SR = 44100.0


def case(T, centres, fbs, depths, mixes, gain, seed, rates=None):
    g = np.random.default_rng(seed)
    B = len(fbs)
    x = gain * (0.6 * np.sin(2 * np.pi * 220 * np.arange(T) / SR)[None, :] + g.uniform(-0.4, 0.4, (B, T)))
    params = {"depth": np.asarray(depths, np.float32), "centre_frequency_hz": np.asarray(centres, np.float32),
              "feedback": np.asarray(fbs, np.float32), "mix": np.asarray(mixes, np.float32)}
    ng = (T + 3) // 4
    if rates is None:                                  # a fast external LFO, so that short clips see the cut-off move
        t = np.arange(ng)[None, :] / ng
        mod = (0.5 + 0.5 * np.sin(2 * np.pi * (2 + np.arange(B))[:, None] * t + g.uniform(0, 6, (B, 1)))).astype(np.float32)
        osc = (np.float32(1.0) - np.float32(2.0) * mod).astype(np.float32)
    else:
        osc, _ = builtin_osc(np.asarray(rates, np.float32), ng, SR)
    return x.astype(np.float32), osc, params, g.standard_normal((B, T))


def autograd64(x, osc, params, dy):
    """d sum(dy * y) by torch autograd in float64; mod = (1 - osc) / 2 is the leaf the LFO gradient refers to."""
    B, T = x.shape
    X = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    MOD = ((1.0 - torch.tensor(osc, dtype=torch.float64)) / 2.0).requires_grad_(True)
    P = {k: torch.tensor(params[k].astype(np.float64), requires_grad=True) for k in PARAMS}
    from tests.helpers.phaser_adjoint64 import log_range
    log_min, log_max = (float(v) for v in log_range(SR))
    span = log_max - log_min
    nc = (torch.log10(P["centre_frequency_hz"]) - log_min) / span
    pre = (1.0 - 2.0 * MOD) * (P["depth"][:, None] / 2.0) + nc[:, None]
    lfo = torch.clamp(pre, 0.0, 1.0)
    g = torch.tan(math.pi * 10.0 ** (lfo * span + log_min) / SR)
    G = g / (1.0 + g)
    s = [torch.zeros(B, dtype=torch.float64) for _ in range(6)]
    last = torch.zeros(B, dtype=torch.float64)
    ms = []
    for n in range(T):
        out = X[:, n] - last
        for k in range(6):
            v = G[:, n >> 2] * (out - s[k])
            yk = v + s[k]
            s[k] = v + yk
            out = 2.0 * yk - out
        last = out * P["feedback"]
        ms.append(out * P["mix"] + X[:, n] * (1.0 - P["mix"]))
    m = torch.stack(ms, 1)
    (torch.clamp(m, -1.0, 1.0) * torch.tensor(dy)).sum().backward()
    out = {"dx": X.grad.numpy(), "dmod": MOD.grad.numpy()}
    out.update({k: v.grad.numpy() for k, v in P.items()})
    return out, m.detach().numpy(), pre.detach().numpy()


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def test_fp32_forward_matches_oracle():
    T = 6001                                            # a last group that is not full
    rates = [0.5, 3.0, 1.7, 2.2]
    x, osc, params, _ = case(T, [70.0, 440.0, 5000.0, 18000.0], [-0.7, 0.25, 0.7, 0.95], [1.0, 0.2, 1.0, 1.0],
                             [1.0, 0.2, 0.5, 1.0], gain=1.6, seed=1, rates=rates)
    y, lfo = ofx.phaser_np(x, rates, params["depth"], params["centre_frequency_hz"], params["feedback"], params["mix"], SR,
                           want_lfo=True)
    f = forward32(x, osc, params, SR)
    assert np.array_equal(f["lfo"], lfo)
    assert np.array_equal(f["y"], y)
    assert (np.abs(f["m"]) > 1).any() and ((f["pre"] < 0) | (f["pre"] > 1)).any()        # both clips are active


def test_adjoint_matches_autograd():
    T = 701
    for seed, rates in ((2, None), (3, [40.0, 25.0, 60.0, 33.0])):
        x, osc, params, dy = case(T, [70.0, 440.0, 5000.0, 18000.0], [-0.7, 0.25, 0.7, 0.95], [1.0, 0.6, 1.0, 0.8],
                                  [1.0, 0.2, 0.5, 0.9], gain=1.6, seed=seed, rates=rates)
        ref, m, pre = autograd64(x, osc, params, dy)
        got = phaser_adjoint64(x, osc, params, SR, dy)
        f = got["fwd32"]
        assert (np.abs(f["m"]) > 1).mean() > 0.02 and (~got["inside"]).any() and got["inside"].any()
        # the fp64 decisions autograd took are the fp32 ones the helper takes
        assert np.array_equal(np.abs(m) <= 1, got["pass_m"]) and np.array_equal((pre >= 0) & (pre <= 1), got["inside"])
        assert np.abs(np.clip(m, -1, 1) - got["y64"]).max() < 1e-9            # the same fp64 forward
        for k in ("dx", "dmod") + PARAMS:
            assert rel(got[k], ref[k]) < 1e-10, (k, rel(got[k], ref[k]))


def test_adjoint_matches_finite_differences():
    T = 600
    x, osc, params, dy = case(T, [440.0, 2000.0], [0.7, -0.5], [0.8, 0.5], [0.7, 1.0], gain=0.3, seed=5)
    got = phaser_adjoint64(x, osc, params, SR, dy)
    assert np.abs(got["fwd32"]["m"]).max() < 0.9 and got["inside"].all()      # no clip edge to step across
    x64, mod64 = x.astype(np.float64), (1.0 - osc.astype(np.float64)) / 2.0
    p64 = {k: params[k].astype(np.float64) for k in PARAMS}

    def loss(xx, mm, pp):
        return float((forward64(xx, mm, pp["depth"], pp["centre_frequency_hz"], pp["feedback"], pp["mix"], SR) * dy).sum())

    g = np.random.default_rng(6)
    errs = []
    for _ in range(12):
        b = int(g.integers(2))
        for name, arr, n in (("dx", x64, int(g.integers(T))), ("dmod", mod64, int(g.integers(T // 4)))):
            eps = 1e-6
            hi, lo = arr.copy(), arr.copy()
            hi[b, n] += eps
            lo[b, n] -= eps
            fd = (loss(hi, mod64, p64) - loss(lo, mod64, p64)) / (2 * eps) if name == "dx" else \
                (loss(x64, hi, p64) - loss(x64, lo, p64)) / (2 * eps)
            errs.append(abs(fd - got[name][b, n]) / np.abs(got[name]).max())
    for k in PARAMS:
        e = 1e-6 * max(1.0, abs(p64[k][0]))
        hi, lo = dict(p64), dict(p64)
        hi[k] = p64[k] + np.array([e, 0.0])
        lo[k] = p64[k] - np.array([e, 0.0])
        fd = (loss(x64, mod64, hi) - loss(x64, mod64, lo)) / (2 * e)
        errs.append(abs(fd - got[k][0]) / abs(got[k][0]))
    assert max(errs) < 1e-6, max(errs)


def test_adjoint_closed_forms():
    T = 600
    # mix = 0: y = clip(x), so dx = dy where it passes, on every processed sample; nothing else gets gradient
    x, osc, params, dy = case(T, [440.0, 5000.0], [0.7, 0.95], [1.0, 0.5], [0.0, 0.0], gain=0.8, seed=7)
    got = phaser_adjoint64(x, osc, params, SR, dy)
    assert got["pass_m"].all() and np.array_equal(got["dx"], dy)
    for k in ("dmod", "depth", "centre_frequency_hz", "feedback"):
        assert np.abs(got[k]).max() == 0, k
    assert np.abs(got["mix"]).min() > 0
    # depth = 0: the LFO does not reach the cut-off
    x, osc, params, dy = case(T, [440.0, 5000.0], [0.7, 0.95], [0.0, 0.0], [1.0, 0.5], gain=1.6, seed=8)
    got = phaser_adjoint64(x, osc, params, SR, dy)
    assert np.abs(got["dmod"]).max() == 0
    assert np.abs(got["centre_frequency_hz"]).min() > 0 and np.abs(got["depth"]).min() > 0


def test_mod_is_the_reference_ground_truth_lfo():
    """The external LFO's convention: with mod = the reference's phaser ground truth make_mod_signal(n, sr, rate, pi / 2,
    "cos") (datasets.py:442; here the oracle's restatement) sampled every 4th sample, osc = 1 - 2 mod reproduces the lfo of
    the built-in oscillator (depth 1, centre in the middle of the log axis, where lfo = (osc + 1) / 2).
    "cos" is (cos(arg + pi) + 1) / 2 (modulations.py:35), so the ground truth is (1 + sin wt) / 2, and JUCE's oscillator is
    sin(phase - pi) = -sin(phase): hence osc = 1 - 2 mod, not 2 mod - 1.
    Measured over 3 s: max |lfo_ext - lfo_builtin| = 5.5e-4 at 0.5 Hz, 8.7e-4 at 1.7 Hz, 1.05e-3 at 3 Hz.  Of the last,
    pi rate / sr = 2.1e-4 is the ground truth's argument running one sample ahead (its cumsum starts at one step, JUCE's
    phase at 0); the rest is fp32 phase drift on both sides (the ground truth's fp32 argument reaches 57 rad, one ulp
    4e-6 rad, times 33 075 accumulated steps of JUCE's phase).  Gate 1.05e-2 = 10x the worst measured value."""
    n = 3 * 44100
    ng = (n + 3) // 4
    worst = 0.0
    for rate in (0.5, 1.7, 3.0):
        mod = omod.make_mod_signal(n, SR, rate, math.pi / 2, "cos").numpy()[::4]
        osc_b, _ = builtin_osc(np.asarray([rate], np.float32), ng, SR)
        centre = np.asarray([math.sqrt(20.0 * 20000.0)], np.float32)
        one = np.ones(1, np.float32)
        _, lfo_b, _ = chain32(osc_b, one, centre, SR)
        _, lfo_e, _ = chain32((np.float32(1.0) - np.float32(2.0) * mod)[None, :], one, centre, SR)
        err = float(np.abs(lfo_e - lfo_b).max())
        print(f"rate {rate}: max |lfo_ext - lfo_builtin| = {err:.3e} (one-sample lead alone: {math.pi * rate / SR:.3e})")
        worst = max(worst, err)
        assert np.abs(lfo_b - 0.5).max() > 0.49                                  # the lfo really swings
    assert worst < 1.05e-2

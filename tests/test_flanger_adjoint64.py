"""CPU: the fp64 flanger adjoint (tests/helpers/flanger_adjoint64.py) against
  (a) torch autograd in float64 through the reference loop (fx.py:92-119) restated without in-place writes (the delay
      line as a python list of per-slot tensors), with the fp32 slots and fractions fed in straight-through;
  (b) central finite differences of the fp64 forward at 40 positions away from floor switches;
  (c) closed forms: fb = depth = 0 (dx = g_z ((1 - mix) + mix), dmod = 0) and mix = 0 (only x and mix get gradient).
Flanger M = 485 (1 + 10 ms) and chorus M = 1764 (40 ms) at 44.1 kHz with N > 2M (the ring wraps), all six continuous LFO
shapes, feedback up to 0.95, min_delay_width = 0 and input levels that clip.

Gates: autograd 1e-10 of max |g| (dx, dmod) and 1e-10 relative (parameters); finite differences 1e-6 relative."""
import numpy as np
import pytest
import torch

from oracle import fx as ofx
from tests.helpers.flanger_adjoint64 import bookkeeping, flanger_adjoint64, forward

SR = 44100.0
SHAPES = ["cos", "rect_cos", "inv_rect_cos", "tri", "saw", "rsaw"]


def lfo(shape, n, freq, phase, exp=1.0):
    """the six continuous shapes of modulations.py, in numpy (values in [0, 1])."""
    t = np.arange(n) / SR
    ph = (2 * np.pi * freq * t + phase) % (2 * np.pi)
    u = ph / (2 * np.pi)
    y = {"cos": (np.cos(ph) + 1) / 2, "rect_cos": np.abs(np.cos(ph)), "inv_rect_cos": 1 - np.abs(np.cos(ph)),
         "tri": 1 - np.abs(2 * u - 1), "saw": u, "rsaw": 1 - u}[shape]
    return (y ** exp).astype(np.float32)


def case(M_min, M_lfo, N, fbs, mdws, mixes, shapes, gain, seed, exp=1.0, freq=3.0):
    g = np.random.default_rng(seed)
    B = len(fbs)
    x = (gain * (0.6 * np.sin(2 * np.pi * 220 * np.arange(N) / SR)[None, :] + g.uniform(-0.4, 0.4, (B, N))))
    x = x.astype(np.float32)
    mod = np.stack([lfo(s, N, freq * (1 + 0.3 * i), g.uniform(0, 2 * np.pi), exp) for i, s in enumerate(shapes)])
    consts = ofx.derive_params(B, M_min, M_lfo, torch.tensor(fbs, dtype=torch.float32),
                               torch.tensor(mdws, dtype=torch.float32), torch.ones(B), torch.tensor([0.8] * B),
                               torch.tensor(mixes, dtype=torch.float32))
    dy = g.standard_normal((B, N))
    return x, mod, consts, M_min + M_lfo, dy


def autograd64(x, mod, consts, M, dy):
    """d sum(dy * y) by torch autograd through the loop without in-place writes (B <= 3)."""
    B, N = x.shape
    w, prev, nxt, frac = bookkeeping(mod, consts, M)
    X = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    MOD = torch.tensor(mod, dtype=torch.float64, requires_grad=True)
    P = {k: torch.tensor(np.asarray(consts[k], np.float64), requires_grad=True)
         for k in ("lfo_scale", "min_delay", "feedback", "depth", "mix")}
    omm = 1.0 - P["mix"]
    r = (torch.tensor(w, dtype=torch.float64)[None, :] - (P["lfo_scale"][:, None] * MOD + P["min_delay"][:, None]) + M) % M
    f = torch.tensor(frac, dtype=torch.float64) + (r - r.detach())          # fp32 value, derivative 1 w.r.t. r
    ring = [None] * M
    zero = torch.zeros((), dtype=torch.float64)
    outs = []
    for n in range(N):
        a = torch.stack([ring[prev[b, n]][b] if ring[prev[b, n]] is not None else zero for b in range(B)])
        c = torch.stack([ring[nxt[b, n]][b] if ring[nxt[b, n]] is not None else zero for b in range(B)])
        v = f[:, n] * c + (1.0 - f[:, n]) * a
        ring[w[n]] = X[:, n] + P["feedback"] * v
        outs.append(X[:, n] + P["depth"] * v)
    o = torch.stack(outs, 1)
    z = omm[:, None] * X + P["mix"][:, None] * o
    y = torch.clamp(z, -1.0, 1.0)
    (y * torch.tensor(dy)).sum().backward()
    out = {"dx": X.grad.numpy(), "dmod": MOD.grad.numpy()}
    out.update({k: v.grad.numpy() for k, v in P.items()})
    return out, z.detach().numpy()


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("M_min,M_lfo,N,shapes,fbs,mdws,exp", [
    (44, 441, 1100, ["cos", "tri", "saw"], [0.0, 0.7, 0.95], [1.0, 0.0, 0.5], 1.0),
    (44, 441, 1100, ["rect_cos", "inv_rect_cos", "rsaw"], [0.3, 0.95, 0.5], [0.0, 1.0, 0.25], 2.0),
    (0, 1764, 3700, ["cos", "saw", "inv_rect_cos"], [0.95, 0.3, 0.0], [0.0, 0.0, 0.0], 1.0),
])
def test_adjoint_matches_autograd(M_min, M_lfo, N, shapes, fbs, mdws, exp):
    x, mod, consts, M, dy = case(M_min, M_lfo, N, fbs, mdws, [1.0, 0.5, 0.25], shapes, gain=1.6, seed=N + M_min, exp=exp)
    ref, z = autograd64(x, mod, consts, M, dy)
    got = flanger_adjoint64(x, mod, consts, M, dy)
    assert (np.abs(got["fwd"]["z32"]) > 1).mean() > 0.02                   # clipping is active
    assert np.abs(got["fwd"]["z"] - z).max() < 1e-12
    for k in ("dx", "dmod"):
        assert rel(got[k], ref[k]) < 1e-10, k
    for k in ("lfo_scale", "min_delay", "feedback", "depth", "mix"):
        assert rel(got[k], ref[k]) < 1e-10, k


def test_adjoint_matches_finite_differences():
    N = 1100
    x, mod, consts, M, dy = case(44, 441, N, [0.7, 0.3], [0.5, 0.0], [1.0, 0.5], ["cos", "tri"], gain=0.4, seed=7)
    got = flanger_adjoint64(x, mod, consts, M, dy)
    book = bookkeeping(mod, consts, M)
    w, prev, nxt, frac = book
    c64 = {k: np.asarray(v, np.float64) for k, v in consts.items()}
    base_r = None

    def loss(xx, mm, cc):
        # fractions move with the fp64 read position (derivative 1), the slots stay those of the fp32 bookkeeping
        r = lambda m_, c_: np.arange(N)[None, :] - (c_["lfo_scale"][:, None] * m_ + c_["min_delay"][:, None])
        f64 = frac.astype(np.float64) + (r(mm, cc) - base_r)
        cc = dict(cc, one_minus_mix=1.0 - cc["mix"])
        return float((forward(xx, None, cc, M, book, f64)["y"] * dy).sum())

    mod64, x64 = mod.astype(np.float64), x.astype(np.float64)
    base_r = np.arange(N)[None, :] - (c64["lfo_scale"][:, None] * mod64 + c64["min_delay"][:, None])
    g = np.random.default_rng(3)
    assert np.abs(got["fwd"]["z32"]).max() < 1                              # no clip boundary to step across
    pos = [(int(g.integers(2)), int(n)) for n in g.integers(2 * M, N, 200)]
    pos = [(b, n) for b, n in pos if 0.02 < frac[b, n] < 0.98][:20]
    assert len(pos) == 20
    eps = 1e-6
    errs = []
    for b, n in pos:
        for name, arr in (("dx", x64), ("dmod", mod64)):
            hi, lo = arr.copy(), arr.copy()
            hi[b, n] += eps
            lo[b, n] -= eps
            args = (hi, mod64, c64) if name == "dx" else (x64, hi, c64)
            argl = (lo, mod64, c64) if name == "dx" else (x64, lo, c64)
            fd = (loss(*args) - loss(*argl)) / (2 * eps)
            errs.append(abs(fd - got[name][b, n]) / max(abs(got[name]).max(), 1e-30))
    for k in ("lfo_scale", "min_delay", "feedback", "depth", "mix"):
        e = 1e-6 * max(1.0, abs(c64[k][0]))
        hi, lo = dict(c64), dict(c64)
        hi[k] = c64[k] + np.array([e, 0.0])
        lo[k] = c64[k] - np.array([e, 0.0])
        fd = (loss(x64, mod64, hi) - loss(x64, mod64, lo)) / (2 * e)
        errs.append(abs(fd - got[k][0]) / max(abs(got[k][0]), 1e-30))
    assert max(errs) < 1e-6


def test_adjoint_closed_forms():
    N = 1100
    x, mod, consts, M, dy = case(44, 441, N, [0.0, 0.0], [1.0, 0.0], [0.25, 1.0], ["cos", "saw"], gain=1.6, seed=11)
    consts["depth"] = np.zeros(2, np.float32)
    got = flanger_adjoint64(x, mod, consts, M, dy)
    gz = np.where(np.abs(got["fwd"]["z32"]) <= 1, dy, 0.0)
    mix = consts["mix"].astype(np.float64)[:, None]
    omm = consts["one_minus_mix"].astype(np.float64)[:, None]
    assert np.abs(got["dx"] - gz * (omm + mix)).max() == 0
    assert np.abs(got["dmod"]).max() == 0
    for k in ("lfo_scale", "min_delay", "feedback"):
        assert np.abs(got[k]).max() == 0, k
    assert np.array_equal(got["depth"], (mix * gz * got["fwd"]["v"]).sum(1))     # d depth = sum g_o v even at depth 0
    # mix = 0: only x and mix receive gradient
    x, mod, consts, M, dy = case(44, 441, N, [0.7, 0.95], [0.5, 0.0], [0.0, 0.0], ["tri", "rsaw"], gain=1.6, seed=12)
    got = flanger_adjoint64(x, mod, consts, M, dy)
    gz = np.where(np.abs(got["fwd"]["z32"]) <= 1, dy, 0.0)
    assert np.abs(got["dx"] - gz).max() == 0
    for k in ("dmod", "lfo_scale", "min_delay", "feedback", "depth"):
        assert np.abs(got[k]).max() == 0, k
    assert np.abs(got["mix"]).min() > 0


def test_fp32_forward_matches_oracle():
    x, mod, consts, M, dy = case(44, 441, 1100, [0.7, 0.95], [0.5, 0.0], [0.5, 1.0], ["cos", "saw"], gain=1.6, seed=5)
    y = ofx.flanger_np(x, mod, consts, M)
    assert np.array_equal(forward(x, mod, consts, M)["y32"], y)

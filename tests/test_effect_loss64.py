"""CPU: the fp64 references of tests/helpers/effect_loss64.py (the yardstick of tests/test_gpu_effect_loss_units.py) against torch
autograd in fp64 through the oracle's loss modules and against central finite differences; the bounds against an fp32 run of the
same formulae, and against seeded defects of that run."""
import numpy as np
import pytest
import torch
from torch import nn

from oracle import losses as ol
from tests.helpers import effect_loss64 as E
from tests.helpers.gpu_harness import ratio

f32, f64 = np.float32, np.float64
WEIGHTS = {"l1": (1.0, 0.0, 0.0, 0.0), "mse": (0.0, 1.0, 0.0, 0.0), "esr": (0.0, 0.0, 1.0, 0.0), "dc": (0.0, 0.0, 0.0, 1.0),
           "mix": (0.3, 0.7, 0.4, 2.0)}


def _autograd(a, t, w, eps):
    """(value, d value / d a) in fp64 through nn.L1Loss, nn.MSELoss, oracle ESRLoss / DCLoss on (B, 1, T)."""
    x = torch.from_numpy(a.astype(f64))[:, None, :].requires_grad_(True)
    y = torch.from_numpy(t.astype(f64))[:, None, :]
    w = [float(f32(v)) for v in w]
    e = float(f32(eps))
    mods = (nn.L1Loss(), nn.MSELoss(), ol.ESRLoss(eps=e), ol.DCLoss(eps=e))
    value = sum(wk * m(x, y) for wk, m in zip(w, mods) if wk != 0.0)
    value.backward()
    return float(value), x.grad[:, 0, :].numpy()


@pytest.mark.parametrize("name", list(WEIGHTS))
@pytest.mark.parametrize("eps", [1e-8, 1e-3])
def test_grad64_against_autograd(name, eps):
    """Each term alone and the mix, on a batch with an ordinary clip (with ties), a silent target and a DC offset."""
    a, t = E.clips(("ordinary", "silent", "dc"), 257, 3)
    assert (a[0] == t[0]).sum() >= 50 and not t[1].any()
    w = WEIGHTS[name]
    r = E.grad64(a, t, 3, *w, eps)
    value, want = _autograd(a, t, w, eps)
    scale = np.abs(want).max(1, keepdims=True)
    assert scale.min() > 0
    assert (np.abs(r["grad"] - want) <= 1e-13 * scale).all()
    assert abs(E.loss64(a, t, *[float(f32(v)) for v in w], float(f32(eps))) - value) <= 1e-13 * abs(value)
    if name in ("l1", "mse", "esr"):
        assert not r["grad"][a == t].any()                            # sign(0) = 0: nothing arrives at a tie


def test_grad64_on_an_all_equal_clip():
    a, t = E.clips(("equal", "ordinary"), 64, 4)
    for name, w in WEIGHTS.items():
        r = E.grad64(a, t, 2, *w, 1e-8)
        assert not r["grad"][0].any() and not r["bound"][0].any(), name
        assert np.abs(r["grad"][1]).max() > 0


@pytest.mark.parametrize("name", list(WEIGHTS))
def test_grad64_against_finite_differences(name):
    """A 7-sample clip pair in a batch of 2, no ties: every term is piecewise linear or quadratic in a, so a central difference
    with h below every |a - t| is exact up to the rounding of the fp64 values (1e-16 / h)."""
    g = np.random.default_rng(7)
    t = g.standard_normal((2, 7)).astype(f32)
    a = (t + np.where(g.random((2, 7)) < 0.5, -1.0, 1.0) * g.uniform(0.05, 0.5, (2, 7))).astype(f32)
    w = [float(f32(v)) for v in WEIGHTS[name]]
    eps = float(f32(1e-3))
    r = E.grad64(a, t, 2, *w, eps)
    h = 1e-5
    assert np.abs(a.astype(f64) - t).min() > 10 * h
    fd = np.zeros((2, 7))
    for b in range(2):
        for i in range(7):
            up, dn = a.astype(f64), a.astype(f64)
            up[b, i] += h
            dn[b, i] -= h
            fd[b, i] = (E.loss64(up, t, *w, eps) - E.loss64(dn, t, *w, eps)) / (2 * h)
    assert np.abs(fd - r["grad"]).max() <= 1e-9 * np.abs(r["grad"]).max()


def test_coefficients():
    """The coefficients by hand on a two-sample clip: t = (1, -2), a = (1.5, -2): S_tt = 5, S_e = -0.5."""
    a, t = np.array([[1.5, -2.0]], f32), np.array([[1.0, -2.0]], f32)
    r = E.grad64(a, t, 1, 1.0, 1.0, 1.0, 1.0, 0.5)
    assert r["c_l1"] == 0.5 and r["c_mse"] == 1.0
    assert r["c_esr"][0] == 2.0 / 5.5                                   # eps beside the SUM of t^2
    assert r["c_dc"][0] == -2.0 * (-0.25) / (2.0 * (2.5 + 0.5))        # eps beside the MEAN of t^2
    assert np.array_equal(r["grad"][0], [0.5 + (1.0 + 2.0 / 5.5) * 0.5 + r["c_dc"][0], r["c_dc"][0]])


def test_sums64_and_terms64():
    a, t = E.clips(("ordinary", "equal", "silent"), 65, 5)
    s, b = E.sums64(a, t)
    e = t.astype(f64) - a.astype(f64)
    assert np.array_equal(s[:, 0], np.abs(e).sum(1)) and np.array_equal(s[:, 3], e.sum(1))
    assert not s[1, [0, 1, 3]].any() and not b[1, [0, 1, 3]].any() and s[2, 2] == 0 and b[2, 2] == 0
    a, t = E.clips(("ordinary", "dc"), 256, 6)
    x, y = torch.from_numpy(a.astype(f64))[:, None], torch.from_numpy(t.astype(f64))[:, None]
    eps = float(f32(1e-3))
    want = {"l1": nn.L1Loss()(x, y), "mse": nn.MSELoss()(x, y), "esr": ol.ESRLoss(eps)(x, y), "dc": ol.DCLoss(eps)(x, y)}
    for k, (v, bound) in E.terms64(a, t, eps).items():
        assert abs(v - float(want[k])) <= 1e-13 * abs(v) and 0 < bound < 1e-6 * v, k


SHAPES = [(1, 1), (1, 63), (1, 64), (2, 65), (3, 255), (2, 256), (3, 257), (2, 1000), (1, 4097)]


def _cases():
    for B, T in SHAPES:
        for v, kinds in enumerate(E.KINDS_BY_B[B]):
            a, t = E.clips(kinds, T, 1000 * T + 10 * B + v)
            prev = np.random.default_rng(T + v).standard_normal((B, T)).astype(f32)
            yield B, T, kinds, a, t, prev


def test_an_fp32_run_meets_the_bounds():
    """The bounds are attainable: numpy's fp32 run of the formulae (sums in fp64, everything else rounded to fp32) stays
    within them on every clip of every shape the GPU test uses, and so do the fp32-difference sums."""
    worst_g, worst_s = 0.0, 0.0
    for B, T, kinds, a, t, prev in _cases():
        e = t - a
        got = np.stack([np.abs(e).astype(f64).sum(1), (e.astype(f64) ** 2).sum(1), (t.astype(f64) ** 2).sum(1),
                        e.astype(f64).sum(1)], 1).astype(f32)
        s, b = E.sums64(a, t)
        worst_s = max(worst_s, ratio(got, s, b))
        for w in WEIGHTS.values():
            for eps in (1e-8, 1e-3):
                for p in (None, prev):
                    r = E.grad64(a, t, B, *w, eps, prev=p)
                    worst_g = max(worst_g, ratio(E.emulate_grad32(a, t, *w, eps, prev=p), r["grad"], r["bound"]))
    print("[measured] effect loss fp32 run: worst ratio sums", round(worst_s, 3), "grad", round(worst_g, 3))
    assert worst_s <= 1.0
    assert worst_g <= 1.0


DEFECTS = {
    "dc_eps_on_the_sum": ("dc", lambda c, B, T, s_tt, s_e, w, eps: dict(c_dc=-2 * w[3] / (B * T) * (s_e / T) / (s_tt + eps))),
    "esr_eps_on_the_mean": ("esr", lambda c, B, T, s_tt, s_e, w, eps: dict(c_esr=2 * w[2] / B / (s_tt + eps * T))),
    "esr_over_BT": ("esr", lambda c, B, T, s_tt, s_e, w, eps: dict(c_esr=c["c_esr"] / T)),
    "dc_sign": ("dc", lambda c, B, T, s_tt, s_e, w, eps: dict(c_dc=-c["c_dc"])),
    "mse_without_the_2": ("mse", lambda c, B, T, s_tt, s_e, w, eps: dict(c_mse=c["c_mse"] / 2)),
    "l1_over_T": ("l1", lambda c, B, T, s_tt, s_e, w, eps: dict(c_l1=c["c_l1"] * B)),
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_defects_are_seen(defect):
    """Each seeded defect of a coefficient leaves the bound both with its term alone and inside the mix, at eps = 1e-3, on a
    batch of loud clips (B = 2 so that 1 / B and 1 / (B T) differ from 1 and 1 / T)."""
    name, change = DEFECTS[defect]
    B, T = 2, 1000
    a, t = E.clips(("ordinary", "dc"), T, 11)
    for wname in (name, "mix"):
        w = [f64(f32(v)) for v in WEIGHTS[wname]]
        eps = f64(f32(1e-3))
        r = E.grad64(a, t, B, *w, eps)
        s_tt, s_e = (t.astype(f64) ** 2).sum(1), (t.astype(f64) - a).sum(1)
        c = dict(r, **change(r, B, T, s_tt, s_e, w, eps))
        d = a.astype(f64) - t
        bad = (c["c_l1"] * np.sign(d) + (c["c_mse"] + c["c_esr"])[:, None] * d + c["c_dc"][:, None]).astype(f32)
        assert ratio(bad, r["grad"], r["bound"]) > 1.0, wname
        for b in range(B):
            assert ratio(bad[b], r["grad"][b], r["bound"][b]) > 1.0, (wname, b)

"""fp64 references and rounding bounds for csrc/effect_loss.hip (mx_effect_loss_sums, mx_effect_loss_grad), written from the
loss definitions (oracle/losses.py; the reference's losses.py:14-67 and nn.L1Loss / nn.MSELoss), not from the kernels.

With a the prediction and t the target, (B, T), every loss with 'mean' reduction over the B clips:
    L1  = 1/(B T) sum |a - t|                                   MSE = 1/(B T) sum (a - t)^2
    ESR = 1/B sum_b  sum_i (t - a)^2 / (sum_i t^2 + eps)        DC  = 1/B sum_b  (mean_i (t - a))^2 / (mean_i t^2 + eps)
so, with d = a - t and per clip S_tt = sum t^2, S_e = sum (t - a):
    dL1/da  = c_l1 sign(d),  c_l1  = w_l1 / (B T)               (sign(0) = 0, as torch's L1 backward has it)
    dMSE/da = c_mse d,       c_mse = 2 w_mse / (B T)
    dESR/da = c_esr d,       c_esr = 2 w_esr / (B (S_tt + eps))
    dDC/da  = c_dc,          c_dc  = -2 w_dc (S_e / T) / (B T (S_tt / T + eps))
The inputs are fp32 numbers; the weights and eps reach the kernel as fp32, so the references take fl32(w), fl32(eps).

Bounds, u = 2^-24 (the unit roundoff of fp32: fl(x) = x (1 + delta), |delta| <= u).

Sums.  The kernel forms e = fl(t - a) = (t - a)(1 + delta) in fp32, squares and accumulates in fp64 (T <= 2^13 terms of relative
error 2^-53 each: below 2^-40 of the magnitude sum, nothing beside u) and rounds every sum once to fp32.
    sum |e|   : u S_abs from the differences, u S_abs (1 + u) from the final rounding                   -> 2 u S_abs
    sum e^2   : (1 + delta)^2: 2 u S_sq, the final rounding u S_sq, the u^2 terms                       -> 4 u S_sq
    sum t^2   : the fp64 products of fp32 numbers are exact; the final rounding u S_tt                  -> 2 u S_tt
    sum e     : sum |t - a| u from the differences, then u |S_e + that| from the final rounding         -> u S_abs + 2 u |S_e|
A clip with a == t has S_abs = 0: the bound is 0 and the three error sums must be exactly 0; a silent target likewise in S_tt.

Gradient, per element: g = fl(fl(fl(c_l1 sgn) + fl(fl(c_mse + c_esr) fl(d))) + c_dc).  One rounding for d, one for each
coefficient (computed in fp64, rounded to fp32), one for c_mse + c_esr, one for the product, two for the adds:
    l1 term at most 3 u, the d term at most 6 u, the dc term at most 2 u of their magnitudes                 -> 8 u of the sum
    bound = 8 u (|c_l1| [d != 0] + (|c_mse| + |c_esr|) |d| + |c_dc|)
accumulate = 1 adds the gradient to the previous content o in fp32: one more rounding of o + g               -> + u (|o| + |g|)
An element with d == 0 in a clip with c_dc == 0 has bound 0: the kernel must write exactly 0 (or exactly o).
"""
import numpy as np

U24 = 2.0 ** -24
f32, f64 = np.float32, np.float64


def _in64(a, t):
    a, t = np.asarray(a), np.asarray(t)
    assert a.dtype == np.float32 and t.dtype == np.float32 and a.shape == t.shape and a.ndim == 2
    return a.astype(f64), t.astype(f64)


def sums64(a, t):
    """(sums (B, 4), bounds (B, 4)) in the order of the kernel's part rows: sum |e|, sum e^2, sum t^2, sum e, e = t - a."""
    a, t = _in64(a, t)
    e = t - a                                                        # exact: fp32 differences fit in fp64 at these magnitudes
    s_abs, s_sq, s_tt, s_e = np.abs(e).sum(1), (e * e).sum(1), (t * t).sum(1), e.sum(1)
    sums = np.stack([s_abs, s_sq, s_tt, s_e], 1)
    bounds = np.stack([2 * U24 * s_abs, 4 * U24 * s_sq, 2 * U24 * s_tt, U24 * s_abs + 2 * U24 * np.abs(s_e)], 1)
    return sums, bounds


def terms64(a, t, eps):
    """The four loss values in fp64 (per-clip ratios first, then the mean) and the error each inherits from the sums' bounds:
    {name: (value, propagated bound)}."""
    B, T = np.asarray(a).shape
    s, b = sums64(a, t)
    eps = f64(f32(eps))
    den_esr, den_dc = s[:, 2] + eps, s[:, 2] / T + eps
    esr, dc = s[:, 1] / den_esr, (s[:, 3] / T) ** 2 / den_dc
    return {
        "l1": (s[:, 0].sum() / (B * T), b[:, 0].sum() / (B * T)),
        "mse": (s[:, 1].sum() / (B * T), b[:, 1].sum() / (B * T)),
        "esr": (esr.mean(), (b[:, 1] / den_esr + esr * b[:, 2] / den_esr).mean()),
        "dc": (dc.mean(), (2 * np.abs(s[:, 3]) * b[:, 3] / T ** 2 / den_dc + b[:, 3] ** 2 / T ** 2 / den_dc
                           + dc * (b[:, 2] / T) / den_dc).mean()),
    }


def loss64(a, t, w_l1, w_mse, w_esr, w_dc, eps):
    """The weighted loss value in fp64 (for finite differences); a, t any float arrays (B, T)."""
    a, t = np.asarray(a, f64), np.asarray(t, f64)
    e = t - a
    l1, mse = np.abs(e).mean(), (e * e).mean()
    esr = ((e * e).sum(1) / ((t * t).sum(1) + eps)).mean()
    dc = (e.mean(1) ** 2 / ((t * t).mean(1) + eps)).mean()
    return w_l1 * l1 + w_mse * mse + w_esr * esr + w_dc * dc


def grad64(a, t, B, w_l1, w_mse, w_esr, w_dc, eps, prev=None):
    """dict(c_l1, c_mse: scalars; c_esr, c_dc: (B,); grad, bound: (B, T)).  ``prev``: the content of dy before an accumulate = 1
    launch (grad and bound then include it)."""
    a, t = _in64(a, t)
    assert a.shape[0] == B
    T = a.shape[1]
    w_l1, w_mse, w_esr, w_dc, eps = (f64(f32(v)) for v in (w_l1, w_mse, w_esr, w_dc, eps))
    d = a - t
    s_tt, s_e = (t * t).sum(1), (t - a).sum(1)
    c_l1, c_mse = w_l1 / (B * T), 2.0 * w_mse / (B * T)
    c_esr = 2.0 * w_esr / (B * (s_tt + eps))
    c_dc = -2.0 * w_dc * (s_e / T) / (B * T * (s_tt / T + eps))
    g = c_l1 * np.sign(d) + (c_mse + c_esr)[:, None] * d + c_dc[:, None]
    bound = 8 * U24 * (abs(c_l1) * (d != 0) + (abs(c_mse) + np.abs(c_esr))[:, None] * np.abs(d) + np.abs(c_dc)[:, None])
    if prev is not None:
        o = np.asarray(prev, f32).astype(f64)
        assert o.shape == g.shape
        bound = bound + U24 * (np.abs(o) + np.abs(g))
        g = g + o
    return dict(c_l1=c_l1, c_mse=c_mse, c_esr=c_esr, c_dc=c_dc, grad=g, bound=bound)


# ---- the inputs of tests/test_gpu_effect_loss_units.py (built here so that the CPU tests see the same clips) --------------------
KINDS_BY_B = {1: (("ordinary",), ("dc",), ("equal",)),
              2: (("ordinary", "silent"), ("dc", "equal")),
              3: (("ordinary", "silent", "dc"), ("equal", "dc", "ordinary"))}


def clips(kinds, T, seed):
    """(a, t) float32 (B, T): one clip per entry of ``kinds``.
    ordinary: independent prediction and target; every fifth sample has prediction == target exactly (sign(0) = 0);
    silent: target all zero;  dc: prediction = fl(target + 0.3);  equal: prediction == target everywhere."""
    g = np.random.default_rng(seed)
    a, t = np.zeros((len(kinds), T), f32), np.zeros((len(kinds), T), f32)
    for b, kind in enumerate(kinds):
        tb = (0.5 * g.standard_normal(T)).astype(f32)
        ab = (tb + 0.2 * g.standard_normal(T).astype(f32)).astype(f32)
        if kind == "ordinary":
            ab[::5] = tb[::5]
        elif kind == "silent":
            tb[:] = 0.0
        elif kind == "dc":
            ab = (tb + f32(0.3)).astype(f32)
            ab[2::7] = tb[2::7]
        elif kind == "equal":
            ab = tb.copy()
        else:
            raise KeyError(kind)
        a[b], t[b] = ab, tb
    return a, t


def emulate_grad32(a, t, w_l1, w_mse, w_esr, w_dc, eps, prev=None):
    """A float32 run of the formulae of the module docstring in the order the bound charges (sums in fp64, every coefficient and
    every per-element operation rounded to fp32): what a correct kernel may produce.  The CPU test holds it to the bound."""
    a, t = np.asarray(a, f32), np.asarray(t, f32)
    B, T = a.shape
    w_l1, w_mse, w_esr, w_dc, eps = (f64(f32(v)) for v in (w_l1, w_mse, w_esr, w_dc, eps))
    s_tt = (t.astype(f64) ** 2).sum(1)
    s_e = (t - a).astype(f64).sum(1)                                   # fp32 differences
    c_l1, c_mse = f32(w_l1 / (B * T)), f32(2.0 * w_mse / (B * T))
    c_esr = (2.0 * w_esr / B / (s_tt + eps)).astype(f32)
    c_dc = (-2.0 * w_dc / (B * T) * (s_e / T) / (s_tt / T + eps)).astype(f32)
    d = a - t
    g = ((c_l1 * np.sign(d)).astype(f32) + ((c_mse + c_esr)[:, None] * d).astype(f32)).astype(f32) + c_dc[:, None]
    g = g.astype(f32)
    return g if prev is None else (g + np.asarray(prev, f32)).astype(f32)

"""CPU: the numpy fp64 restatement of the gain match (tests/helpers/gain_match64.py, K20) -- its backward against central
finite differences of the scalar sum(w * z) at every element, N = 33.

The function that is differentiated is the un-rounded one: z = g * y_hat with g as the formula gives it (``g64``), which is
also the gain handed to the helper's backward; the fp32 rounding of g that the kernels apply is piecewise constant and has
no derivative.  Gate: 1e-6 of max |dy_hat|, the gate of the other adjoint helpers' FD tests.  Steps: 1e-6 on rows of O(0.3)
samples (truncation ~ h^2, rounding ~ 1e-16 / h); 1e-9 on the silent row, where the curvature is 1 / eps = 1e8 and the
truncation error h^2 / eps.  On the silent row under "ls" the gradient is exactly 0 and so is the difference quotient
(f is even in every element there), which the zero gate asks for.
"""
import numpy as np
import pytest

from tests.helpers import gain_match64 as h

N = 33
EPS = 1e-8


def rows(kind, rng):
    """(y_hat, y, gain_range, expected flag) of one case."""
    p = 0.3 * rng.standard_normal(N)
    noise = 0.05 * rng.standard_normal(N)
    if kind == "free":
        return p, 0.6 * p + noise, None, 0
    if kind == "in_range":
        return p, 0.6 * p + noise, (0.05, 20.0), 0
    if kind == "clamp_high":
        return p, 3.0 * p + noise, (0.5, 2.0), 1
    if kind == "clamp_low":
        return p, 0.1 * p + 0.01 * noise, (0.5, 2.0), 1
    if kind == "silent":
        return np.zeros(N), 0.3 * rng.standard_normal(N), None, 0
    raise AssertionError(kind)


def f(p, q, w, mode, rng_):
    a, c, e = float(np.dot(p, p)), float(np.dot(p, q)), float(np.dot(q, q))
    g, _ = h.gain64(a, c, e, mode, EPS, rng_)
    return float(np.dot(w, g * p))


@pytest.mark.parametrize("mode", h.MODES)
@pytest.mark.parametrize("kind", ["free", "in_range", "clamp_high", "clamp_low", "silent"])
def test_backward_against_finite_differences(mode, kind):
    rng = np.random.default_rng(100 + 7 * h.MODES.index(mode) + len(kind))
    p, q, rng_, want_flag = rows(kind, rng)
    w = rng.standard_normal(N)
    fwd = h.forward64(p.astype(np.float32), q.astype(np.float32), mode, EPS, rng_)      # the flag of the fp32 row
    a = float(np.dot(p, p))
    g, flag = h.gain64(a, float(np.dot(p, q)), float(np.dot(q, q)), mode, EPS, rng_)
    assert flag == want_flag == fwd["flag"]
    if kind == "silent":
        assert g == (0.0 if mode == "ls" else float(np.sqrt((np.dot(q, q) + EPS) / EPS)))
    got = h.backward64(w, p, q, g, a, flag, mode, EPS)["dy_hat"]                         # dz = w
    step = 1e-9 if kind == "silent" else 1e-6
    fd = np.empty(N)
    for i in range(N):
        up, dn = p.copy(), p.copy()
        up[i] += step
        dn[i] -= step
        fd[i] = (f(up, q, w, mode, rng_) - f(dn, q, w, mode, rng_)) / (up[i] - dn[i])
    err, top = float(np.abs(fd - got).max()), float(np.abs(got).max())
    print(f"{mode} {kind}: g {g:.6g} flag {flag}, max |fd - dy_hat| {err:.3e}, max |dy_hat| {top:.3e}")
    assert err <= 1e-6 * top


def test_forward_rounds_the_gain_once_and_flags_the_clamp():
    rng = np.random.default_rng(5)
    p = (0.3 * rng.standard_normal(N)).astype(np.float32)
    q = (0.25 * p + 0.01 * rng.standard_normal(N)).astype(np.float32)
    for mode in h.MODES:
        out = h.forward64(p, q, mode, EPS, (0.05, 20.0))
        assert out["flag"] == 0 and out["g32"].dtype == np.float32 and out["g32"] == np.float32(out["g64"])
        assert np.array_equal(out["z64"], float(out["g32"]) * p.astype(np.float64))
        p64, q64 = p.astype(np.float64), q.astype(np.float64)
        assert np.allclose(out["sums"], [np.dot(p64, p64), np.dot(p64, q64), np.dot(q64, q64)], rtol=1e-14, atol=0.0)
        lo = h.forward64(p, q, mode, EPS, (0.5, 2.0))
        assert lo["flag"] == 1 and lo["g32"] == np.float32(0.5)
    inv = h.forward64(p, -q, "ls", EPS, (0.05, 20.0))                                    # an inverted pair: clamped to lo
    assert inv["g64"] == 0.05 and inv["flag"] == 1
    assert h.forward64(p, -q, "rms", EPS, (0.05, 20.0))["flag"] == 0                     # the energy match has no sign
    # a clamped row's backward is g dz alone
    dz = rng.standard_normal(N)
    back = h.backward64(dz, p, q, np.float32(0.5), float(lo["sums"][0]), 1, "ls", EPS)
    assert np.array_equal(back["dy_hat"], 0.5 * dz)
    stacked = h.rows64(np.stack([p, p]), np.stack([q, -q]), "ls", EPS, (0.05, 20.0))
    assert stacked["sums"].shape == (2, 3) and stacked["flag"].tolist() == [0, 1] and stacked["z64"].shape == (2, N)

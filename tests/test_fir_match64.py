"""CPU: the numpy fp64 statement of the per-clip FIR match (tests/helpers/fir_match64.py, K21) against itself.

1. the composition's gradient against central finite differences at EVERY sample, for (N, K, c, ridge) in (40, 1, 0, 0),
   (40, 5, 2, 1e-6), (40, 5, 0, 1e-6), (40, 5, 4, 1e-3), (7, 9, 4, 1e-2), (64, 8, 3, 1e-6).  Gate: 1e-6 of max |grad|.  With
   a step of 1e-5 the truncation error of a central difference of this rational function is ~1e-10 relative and its
   rounding error ~1e-11; measured here: 4.5e-10 at worst (the derivation's own check measured 3.5e-9).
2. K = 1, ridge = 0 is the K20 helper's "ls" gain, forward and backward.
3. a flagged row is the identity forward and backward, for each of the two guards.
4. the stage functions agree with direct definitions written another way (np.convolve, np.linalg.solve).
"""
import numpy as np
import pytest

from tests.helpers import fir_match64 as h
from tests.helpers import gain_match64 as g

FD_CASES = [(40, 1, 0, 0.0), (40, 5, 2, 1e-6), (40, 5, 0, 1e-6), (40, 5, 4, 1e-3), (7, 9, 4, 1e-2), (64, 8, 3, 1e-6)]


def comb_rows(rng, N, level=1.0):
    """x: a noise-driven comb; y: x through a short filter plus noise; dz: noise."""
    src = rng.standard_normal(N + 16)
    x = (src[16:] + 0.7 * src[9:N + 9]) * level
    y = 0.5 * h.shifted(x, 1) + 0.3 * x - 0.1 * h.shifted(x, -2) + 0.05 * level * rng.standard_normal(N)
    return x, y, rng.standard_normal(N)


@pytest.mark.parametrize("N, K, c, ridge", FD_CASES)
def test_gradient_against_central_differences(N, K, c, ridge):
    rng = np.random.default_rng(100 * N + K + c)
    x, y, dz = comb_rows(rng, N)
    eps = 1e-8
    loss = lambda v: float(np.dot(dz, h.forward64(v, y, K, c, ridge, eps, 1e9, round_taps=False)["z64"]))
    fwd = h.forward64(x, y, K, c, ridge, eps, 1e9, round_taps=False)
    assert fwd["flag"] == 0
    grad = h.backward64(dz, x, y, fwd, c, ridge, eps)["dy_hat"]
    step = 1e-5
    fd = np.zeros(N)
    for i in range(N):
        e = np.zeros(N)
        e[i] = step
        fd[i] = (loss(x + e) - loss(x - e)) / (2 * step)
    err = float(np.abs(fd - grad).max() / np.abs(grad).max())
    print(f"N = {N}, K = {K}, c = {c}, ridge = {ridge}: |fd - grad| / max |grad| = {err:.2e}")
    assert err < 1e-6


def test_the_ridge_term_of_s0_matters():
    """Without ``s[0] += 2 ridge <u, h>`` the gradient is off by the order of ridge: the finite-difference gate sees it."""
    N, K, c, ridge = 40, 5, 2, 1e-2
    x, y, dz = comb_rows(np.random.default_rng(7), N)
    fwd = h.forward64(x, y, K, c, ridge, 1e-8, 1e9, round_taps=False)
    back = h.backward64(dz, x, y, fwd, c, ridge, 1e-8)
    s = back["s"].copy()
    s[K - 1] -= 2.0 * ridge * float(np.dot(back["u"], fwd["taps"]))
    wrong = h.bwd_apply(dz, y, x, fwd["taps"], back["u"], s, c)["dy_hat"]
    assert np.abs(wrong - back["dy_hat"]).max() > 1e-4 * np.abs(back["dy_hat"]).max()


def test_one_tap_is_the_ls_gain():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(50).astype(np.float32)
    y = (0.4 * x + 0.1 * rng.standard_normal(50)).astype(np.float32)
    dz = rng.standard_normal(50).astype(np.float32)
    fwd = h.forward64(x, y, 1, 0, 0.0, 1e-8, 20.0)
    ref = g.forward64(x, y, "ls", 1e-8, None)
    assert np.array_equal(fwd["sums"], ref["sums"]) and fwd["taps"][0] == ref["g32"] and fwd["flag"] == 0
    assert np.array_equal(fwd["z64"], ref["z64"])
    back = h.backward64(dz, x, y, fwd, 0, 0.0, 1e-8)
    want = g.backward64(dz, x, y, ref["g32"], ref["sums"][0], 0, "ls", 1e-8)
    assert np.abs(back["dy_hat"] - want["dy_hat"]).max() <= 1e-15 * want["scale"].max()
    assert abs(back["gh"][0] - want["s"]) == 0.0


def test_a_flagged_row_is_the_identity():
    rng = np.random.default_rng(4)
    x, y, dz = comb_rows(rng, 30)
    K, c = 5, 1
    big = h.forward64(x, 1000.0 * y, K, c, 1e-6, 1e-8, 20.0)                    # sum |h| > max_gain
    bad = x.copy()
    bad[3] = np.inf                                                            # R[0] = inf: the first pivot is not finite
    for fwd, src in ((big, x), (h.forward64(bad, y, K, c, 1e-6, 1e-8, 20.0), bad)):
        assert fwd["flag"] in (1, 2) and fwd["taps"].tolist() == [0.0, 1.0, 0.0, 0.0, 0.0]
        assert np.array_equal(fwd["z64"], src)                                 # zero taps read nothing: inf stays inf, no NaN
        back = h.backward64(dz, src, y, fwd, c, 1e-6, 1e-8)
        assert not back["u"].any() and not back["s"].any() and np.array_equal(back["dy_hat"], dz)
    assert big["flag"] == 2 and h.forward64(bad, y, K, c)["flag"] == 1
    quiet = h.forward64(np.zeros(30), y, K, c, 1e-6, 1e-300, 20.0)             # a silent y_hat: h = 0 through eps, no flag
    assert quiet["flag"] == 0 and not quiet["taps"].any() and not quiet["z64"].any()
    assert h.forward64(x, -y, K, c)["flag"] == 0                               # an inverted pair: negative taps, not flagged
    assert np.array_equal(h.forward64(x, -y, K, c)["taps"], -h.forward64(x, y, K, c)["taps"])


def test_stages_against_direct_definitions():
    rng = np.random.default_rng(5)
    N, K, c = 23, 6, 2
    x, y, dz = comb_rows(rng, N)
    xp = np.concatenate([np.zeros(K), x, np.zeros(K)])                         # zero-extended, x[n] at xp[K + n]
    S = h.sums(x, y, K, c)["sums"]
    for d in range(K):
        assert abs(S[d] - sum(x[n] * xp[K + n + d] for n in range(N))) < 1e-12
        assert abs(S[K + d] - sum(xp[K + n + c - d] * y[n] for n in range(N))) < 1e-12
    assert abs(S[2 * K] - np.dot(y, y)) < 1e-12
    sol = h.solve(S, K, c, 1e-3, 1e-8, 1e9, round_taps=False)
    A = h.system(S[:K], 1e-3, 1e-8)
    assert np.allclose(A, A.T) and A[0, 0] == S[0] + (1e-8 + 1e-3 * S[0]) and A[1, 3] == S[2]
    assert np.allclose(sol["h64"], np.linalg.solve(A, S[K:2 * K]), rtol=1e-12, atol=0)
    assert abs(sol["cond"] - np.linalg.cond(A)) < 1e-9 * sol["cond"]
    z = h.apply(x, sol["taps"], c)["z64"]
    assert np.allclose(z, np.convolve(x, sol["taps"])[c:c + N], rtol=0, atol=1e-13)
    # the taps minimise |z - y|^2 + lambda |h|^2 over the zero-extended rows: the normal equations hold
    full = np.convolve(x, sol["taps"])                                          # z on n = -c .. N + K - 2 - c
    target = np.concatenate([np.zeros(c), y, np.zeros(K - 1 - c)])
    resid = full - target
    lam = 1e-8 + 1e-3 * S[0]
    for k in range(K):
        basis = np.concatenate([np.zeros(k), x, np.zeros(K - 1 - k)])
        assert abs(np.dot(resid, basis) + lam * sol["taps"][k]) < 1e-10
    B = h.bwd_sums(dz, x, K, c)
    for k in range(K):
        assert abs(B["gh"][k] - sum(dz[n] * xp[K + n + c - k] for n in range(N))) < 1e-12
    bs = h.bwd_solve(B["gh"], S[:K], sol["taps"], 0, 1e-3, 1e-8)
    assert np.allclose(bs["u"], np.linalg.solve(A, B["gh"]), rtol=1e-12, atol=0)
    assert np.allclose(bs["s"], bs["s"][::-1]) and bs["s"].shape == (2 * K - 1,)
    rows = h.rows64(np.stack([x, 2 * x]), np.stack([y, y]), K, c)
    assert rows["taps"].shape == (2, K) and rows["z64"].shape == (2, N) and rows["flag"].tolist() == [0, 0]
    back = h.rows_backward64(np.stack([dz, dz]), np.stack([x, 2 * x]), np.stack([y, y]), rows, c)
    assert back["dy_hat"].shape == (2, N) and back["u"].shape == (2, K) and back["s"].shape == (2, 2 * K - 1)

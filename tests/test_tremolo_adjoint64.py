"""CPU: the fp64 tremolo adjoint (tests/helpers/tremolo_adjoint64.py) against central finite differences of its fp64
forward, at EVERY point of the low-rate LFO row (and for mix, and for a handful of samples of x).

N = 257 with n_mod = 1 (a constant LFO), 2 (one segment), 7, 256 (one short of full rate: every sample straddles two
points) and 257 (full rate, no resampling).  The forward is linear in each of its inputs, so a central difference has no
truncation error and eps = 1e-4 keeps the cancellation (~1e-16 / eps) at 1e-12.

Gate: 1e-6 of max |dmod|, the finite-difference gate of tests/test_flanger_adjoint64_lr.py."""
import numpy as np
import pytest

from tests.helpers.tremolo_adjoint64 import taps, tremolo_adjoint64, tremolo_forward64, upsample64, upsample_transpose64

EPS = 1e-4
N = 257


def case(n_mod, seed):
    g = np.random.default_rng(seed)
    B = 3
    x = g.uniform(-1.0, 1.0, (B, N)).astype(np.float32)
    mod = g.uniform(0.0, 1.0, (B, n_mod)).astype(np.float32)
    mix = np.array([1.0, 0.37, 0.05], np.float32)
    dy = g.standard_normal((B, N))
    return x, mod, mix, dy


@pytest.mark.parametrize("n_mod", [1, 2, 7, 256, 257])
def test_taps_partition_of_unity_and_transpose(n_mod):
    i0, i1, lam0, lam1 = taps(n_mod, N)
    assert (np.diff(i0) >= 0).all() and i0[0] == 0 and i1[-1] == n_mod - 1 and i1.max() <= n_mod - 1
    assert np.abs(lam0.astype(np.float64) + lam1 - 1.0).max() < 1e-7
    g = np.random.default_rng(n_mod)
    a, b = g.standard_normal((2, n_mod)), g.standard_normal((2, N))
    lhs, rhs = (upsample64(a, N) * b).sum(), (a * upsample_transpose64(b, n_mod)).sum()        # <A a, b> == <a, A^T b>
    assert abs(lhs - rhs) < 1e-9 * max(1.0, abs(lhs))


@pytest.mark.parametrize("n_mod", [1, 2, 7, 256, 257])
def test_adjoint_matches_finite_differences(n_mod):
    x, mod, mix, dy = case(n_mod, seed=100 + n_mod)
    got = tremolo_adjoint64(x, mod, mix, dy)
    mod64, mix64, x64 = mod.astype(np.float64), mix.astype(np.float64), x.astype(np.float64)

    def loss(x_=x64, mod_=mod64, mix_=mix64):
        return float((tremolo_forward64(x_, mod_, mix_) * dy).sum())

    scale = np.abs(got["dmod"]).max()
    assert scale > 0
    worst = 0.0
    for b in range(x.shape[0]):
        for k in range(n_mod):                                              # every point of the row
            hi, lo = mod64.copy(), mod64.copy()
            hi[b, k] += EPS
            lo[b, k] -= EPS
            fd = (loss(mod_=hi) - loss(mod_=lo)) / (2 * EPS)
            err = abs(fd - got["dmod"][b, k]) / scale
            assert err < 1e-6, (b, k, fd, got["dmod"][b, k])
            worst = max(worst, err)
    print("n_mod", n_mod, "worst finite-difference error of dmod", worst)
    for b in range(x.shape[0]):                                             # d mix, the 1 - mix path included
        hi, lo = mix64.copy(), mix64.copy()
        hi[b] += EPS
        lo[b] -= EPS
        fd = (loss(mix_=hi) - loss(mix_=lo)) / (2 * EPS)
        assert abs(fd - got["dmix"][b]) < 1e-6 * np.abs(got["dmix"]).max(), (b, fd, got["dmix"][b])
    for b, n in ((0, 0), (1, 100), (2, N - 1)):
        hi, lo = x64.copy(), x64.copy()
        hi[b, n] += EPS
        lo[b, n] -= EPS
        fd = (loss(x_=hi) - loss(x_=lo)) / (2 * EPS)
        assert abs(fd - got["dx"][b, n]) < 1e-6 * np.abs(got["dx"]).max(), (b, n)


def test_full_rate_is_elementwise():
    x, mod, mix, dy = case(N, seed=5)
    got = tremolo_adjoint64(x, mod, mix, dy)
    assert np.array_equal(got["dmod"], mix.astype(np.float64)[:, None] * (dy * x.astype(np.float64)))

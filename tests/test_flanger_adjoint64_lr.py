"""CPU: the fp64 low-rate flanger adjoint (tests/helpers/flanger_adjoint64_lr.py) against central finite differences of the
fp64 forward, for EVERY point of the low-rate LFO row.

The forward under test is the fp64 forward of tests/helpers/flanger_adjoint64.py fed with the fp64 resampling of the
low-rate row (fp32 taps and weights, fp64 sums); as in tests/test_flanger_adjoint64.py the slots stay those of the fp32
bookkeeping and the read fractions move with the fp64 read position.  That restatement equals the forward itself as long
as no perturbed sample crosses a slot boundary, so the LFO rows are chosen -- and asserted -- to keep every sample's read
fraction at least 2 * lfo_scale * eps away from 0 and 1 (a perturbation of eps of one point moves a read position by at
most lfo_scale * eps).  Flanger (M = 485) and chorus (M = 1764) geometry, n_mod = 11 and 23, N ragged.

Gate: 1e-6 of max |dmod|, the finite-difference gate of tests/test_flanger_adjoint64.py (eps = 1e-7: truncation
~eps^2, cancellation ~1e-16 / eps, both far below it)."""
import numpy as np
import pytest
import torch

from oracle import fx as ofx
from tests.helpers.flanger_adjoint64 import bookkeeping, forward
from tests.helpers.flanger_adjoint64_lr import (flanger_adjoint64_lr, interp_transpose64, taps, upsample32, upsample64)

SR = 44100.0
EPS = 1e-7


def case(M_min, M_lfo, N, n_mod, fbs, mdws, mixes, seed):
    g = np.random.default_rng(seed)
    B = len(fbs)
    x = (0.4 * (0.6 * np.sin(2 * np.pi * 220 * np.arange(N) / SR)[None, :] + g.uniform(-0.4, 0.4, (B, N)))).astype(np.float32)
    consts = ofx.derive_params(B, M_min, M_lfo, torch.tensor(fbs, dtype=torch.float32), torch.tensor(mdws, dtype=torch.float32),
                               torch.ones(B), torch.tensor([0.8] * B), torch.tensor(mixes, dtype=torch.float32))
    dy = g.standard_normal((B, N))
    M = M_min + M_lfo
    margin = 2.0 * float(np.max(consts["lfo_scale"])) * EPS
    # LFO rows away from the slot boundaries: smooth random rows, redrawn until every sample's fraction keeps the margin
    for attempt in range(200):
        t = np.linspace(0.0, 1.0, n_mod)
        mod_lr = np.stack([0.5 + 0.45 * np.sin(2 * np.pi * (g.uniform(0.5, 2.0) * t + g.uniform())) for _ in range(B)])
        mod_lr = mod_lr.astype(np.float32)
        frac = bookkeeping(upsample32(mod_lr, N), consts, M)[3]
        if frac.min() > margin and frac.max() < 1.0 - margin:
            return x, mod_lr, consts, M, dy, margin
    raise AssertionError("no LFO row away from the slot boundaries found")


def test_taps_are_a_partition_of_unity_and_monotonic():
    for n_mod, N in ((11, 1100), (345, 88200), (882, 88200), (1, 7), (7, 7)):
        i0, i1, lam0, lam1 = taps(n_mod, N)
        assert (np.diff(i0) >= 0).all() and i0[0] == 0 and i1[-1] == n_mod - 1
        assert np.abs(lam0.astype(np.float64) + lam1 - 1.0).max() < 1e-7
        ones = interp_transpose64(np.ones((1, N)), n_mod)
        assert abs(ones.sum() - N) < 1e-3                                    # every sample's weight lands somewhere, once


@pytest.mark.parametrize("M_min,M_lfo,N,n_mod", [(44, 441, 1103, 11), (44, 441, 1103, 23), (0, 1764, 3701, 23)])
def test_low_rate_adjoint_matches_finite_differences(M_min, M_lfo, N, n_mod):
    x, mod_lr, consts, M, dy, margin = case(M_min, M_lfo, N, n_mod, [0.7, 0.3], [0.5, 0.0], [1.0, 0.5], seed=N + n_mod)
    got = flanger_adjoint64_lr(x, mod_lr, consts, M, dy)
    book = bookkeeping(got["mod_full"], consts, M)
    frac = book[3]
    assert frac.min() > margin and frac.max() < 1.0 - margin                # every sample, so every perturbed point
    assert np.abs(got["fwd"]["z32"]).max() < 1                              # no clip boundary to step across
    c64 = {k: np.asarray(v, np.float64) for k, v in consts.items()}
    x64, lr64 = x.astype(np.float64), mod_lr.astype(np.float64)
    r = lambda lr: np.arange(N)[None, :] - (c64["lfo_scale"][:, None] * upsample64(lr, N) + c64["min_delay"][:, None])
    base_r = r(lr64)

    def loss(lr):
        f64 = frac.astype(np.float64) + (r(lr) - base_r)
        return float((forward(x64, None, c64, M, book, f64)["y"] * dy).sum())

    scale = np.abs(got["dmod"]).max()
    assert scale > 0
    worst = 0.0
    for b in range(x.shape[0]):
        for k in range(n_mod):                                              # every point of the row
            hi, lo = lr64.copy(), lr64.copy()
            hi[b, k] += EPS
            lo[b, k] -= EPS
            fd = (loss(hi) - loss(lo)) / (2 * EPS)
            err = abs(fd - got["dmod"][b, k]) / scale
            assert err < 1e-6, (b, k, fd, got["dmod"][b, k])
            worst = max(worst, err)
    print("worst finite-difference error", worst)


def test_full_rate_row_is_the_full_rate_adjoint():
    from tests.helpers.flanger_adjoint64 import flanger_adjoint64
    x, mod_lr, consts, M, dy, _ = case(44, 441, 1103, 11, [0.7, 0.3], [0.5, 0.0], [1.0, 0.5], seed=3)
    full = upsample32(mod_lr, 1103)
    a, b = flanger_adjoint64_lr(x, full, consts, M, dy), flanger_adjoint64(x, full, consts, M, dy)
    assert np.array_equal(a["dmod"], b["dmod"]) and np.array_equal(a["dx"], b["dx"])

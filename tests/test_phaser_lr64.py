"""CPU: the fp64 low-rate expand / gather of the phaser LFO (tests/helpers/phaser_lr64.py).

1. gather64 is the transpose of the linear part of expand64: <expand(m) - expand(0), d> == <m, gather(d)> to 1e-12 relative.
2. The composition with the fp64 phaser adjoint (tests/helpers/phaser_adjoint64.py, external LFO): d loss / d mod_lr =
   gather64(dmod at group rate) against central finite differences of the fp64 forward at EVERY low-rate point.  The adjoint
   is evaluated at the fp32-rounded osc row (its contract), so the differences are taken around that same point: the group
   row (1 - osc32) / 2 plus the (linear) expansion of the perturbation.  Gate 1e-6 of max |dmod_lr|, the finite-difference
   gate of tests/test_flanger_adjoint64_lr.py and tests/test_tremolo_adjoint64.py; the worst value is printed.

Shapes (N, n_mod, lead): (1, 1, 0) a single sample and point; (4, 2, 0) one full group; (5, 2, 3) a lead that is not a
multiple of 4 and a clamp at both ends; (37, 5, 6); (64, 64, 1) the identity case n_mod == N behind a lead."""
import numpy as np
import pytest

from tests.helpers import phaser_adjoint64 as pa
from tests.helpers.phaser_lr64 import expand64, gather64, group_samples, taps_at

SR = 44100.0
SHAPES = [(1, 1, 0), (4, 2, 0), (5, 2, 3), (37, 5, 6), (64, 64, 1)]


@pytest.mark.parametrize("N,n_mod,lead", SHAPES)
def test_gather_is_the_transpose_of_expand(N, n_mod, lead):
    g = np.random.default_rng(1000 * N + n_mod)
    B = 3
    leads = [lead, 0, lead + 2]                                               # per-row leads
    width = N + max(leads) + 5                                                # groups beyond every clip
    ng = (width + 3) // 4
    m, d = g.standard_normal((B, n_mod)), g.standard_normal((B, ng))
    lin = expand64(m, leads, N, width) - expand64(np.zeros((B, n_mod)), leads, N, width)
    lhs, rhs = (lin * d).sum(), (m * gather64(d, leads, N, n_mod)).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1e-300), (lhs, rhs)
    # the groups beyond lead + N hold 0.5 and take no gradient; the lead-in holds the first value
    out = expand64(m, leads, N, width)
    for b in range(B):
        n, valid = group_samples(N, leads[b], ng)
        assert valid.sum() == (leads[b] + N + 3) // 4 and (out[b, ~valid] == 0.5).all()
        i0, i1, lam0, lam1 = taps_at(n, n_mod, N)
        assert (np.diff(i0) >= 0).all() and i0.min() >= 0 and i1.max() <= n_mod - 1
        lead_in = 4 * np.arange(ng) <= leads[b]
        assert np.array_equal(out[b, lead_in & valid], np.full(int((lead_in & valid).sum()), m[b, 0]))
    if n_mod == N:                                                            # a plain read
        assert np.array_equal(out[1, :(N + 3) // 4], m[1, ::4])


@pytest.mark.parametrize("N,n_mod,lead", SHAPES)
def test_composition_matches_finite_differences(N, n_mod, lead):
    g = np.random.default_rng(7 + N)
    B, T = 2, lead + N
    leads = [lead] * B
    t = np.arange(T) / SR
    x = (0.3 * (0.5 * np.sin(2 * np.pi * 220.0 * t)[None, :] + g.uniform(-0.4, 0.4, (B, T)))).astype(np.float32)
    params = {"depth": np.asarray([0.8, 0.5], np.float32), "centre_frequency_hz": np.asarray([440.0, 2000.0], np.float32),
              "feedback": np.asarray([0.7, -0.5], np.float32), "mix": np.asarray([0.7, 1.0], np.float32)}
    mod_lr = g.uniform(0.2, 0.8, (B, n_mod)).astype(np.float32)
    dy = np.concatenate([np.zeros((B, lead)), g.standard_normal((B, N))], 1)
    base_g = expand64(mod_lr, leads, N, T)
    osc = (1.0 - 2.0 * base_g).astype(np.float32)
    got = pa.phaser_adjoint64(x, osc, params, SR, dy)
    assert np.abs(got["fwd32"]["m"]).max() < 0.9 and got["inside"].all()      # no clip edge to step across
    dmod_lr = gather64(got["dmod"], leads, N, n_mod)
    scale = np.abs(dmod_lr).max()
    assert scale > 0
    point = (1.0 - osc.astype(np.float64)) / 2.0                              # where the adjoint was evaluated
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    x64, m64 = x.astype(np.float64), mod_lr.astype(np.float64)

    def loss(m):
        mg = point + (expand64(m, leads, N, T) - base_g)
        return float((pa.forward64(x64, mg, p64["depth"], p64["centre_frequency_hz"], p64["feedback"], p64["mix"], SR) * dy).sum())

    eps, worst = 1e-6, 0.0
    for b in range(B):
        for k in range(n_mod):                                                # every point of the row
            hi, lo = m64.copy(), m64.copy()
            hi[b, k] += eps
            lo[b, k] -= eps
            fd = (loss(hi) - loss(lo)) / (2 * eps)
            err = abs(fd - dmod_lr[b, k]) / scale
            worst = max(worst, err)
            assert err < 1e-6, (b, k, fd, dmod_lr[b, k])
    print(f"(N, n_mod, lead) = {(N, n_mod, lead)}: worst finite-difference error of dmod_lr {worst:.3e} of max |dmod_lr| {scale:.3e}")

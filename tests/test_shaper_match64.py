"""CPU: the numpy fp64 restatement of the shaper match (K27, tests/helpers/shaper_match64.py) against independent arithmetic
-- ``numpy.linalg.lstsq`` on the scaled basis, central finite differences of its own forward, the scaling invariances, the
acceptance rows of the issue's table and hand-made rows for every flag.  The device tests hold the kernels to this helper."""
import numpy as np
import pytest

from tests.helpers import shaper_match64 as h

N = 22272
CONFIGS = [(P, even) for P in (1, 3, 5, 7) for even in (False, True)]


def pair(n=4096, seed=0, amp=0.25):
    x = h.comb(n, seed, amp).astype(np.float64)
    y = 0.25 * amp * np.tanh(2.0 * x / amp) + 0.05 * x * x / amp
    return x, y


@pytest.mark.parametrize("order,even", CONFIGS)
def test_coefficients_against_lstsq(order, even):
    """ridge = 0: c is the least-squares solution on the basis t^(p_k) against y / r.  lstsq works on the basis itself (an SVD),
    the helper on its Gram matrix: they agree to cond(A) 2^-53 with a factor of 64 for the K <= 7 steps of either."""
    x, y = pair()
    f = h.forward(x, y, order, even, ridge=0.0, max_gain=1e6, round32=False)
    assert f["flag"] == 0
    t = x / f["r"]
    basis = np.stack([t ** p for p in h.powers(order, even)], 1)
    ref = np.linalg.lstsq(basis, y / f["r"], rcond=None)[0]
    A, _ = h.gram(f["sums"], order, even)
    gate = 64 * np.linalg.cond(A) * 2.0 ** -53 * np.max(np.abs(ref))
    assert np.max(np.abs(f["c"] - ref)) <= gate
    assert np.linalg.cond(A) < 1e7                                  # monomials in x / rms stay well conditioned up to order 7


@pytest.mark.parametrize("order,even", CONFIGS)
def test_backward_against_finite_differences(order, even):
    """d <w, z> / d x by the helper's backward against central differences (the five-point stencil, step 1e-3 rms) of the
    helper's own unrounded forward, r moving with x as it does: gate 1e-6 norm-wise."""
    n = 192
    x, y = pair(n, seed=3)
    w = np.random.default_rng(4).standard_normal(n)
    ridge = 1e-9
    f = h.forward(x, y, order, even, ridge, 1e6, round32=False)
    assert f["flag"] == 0
    got = h.backward(w, x, y, f, order, even, ridge)["dy"]
    loss = lambda v: float(np.dot(w, h.forward(v, y, order, even, ridge, 1e6, round32=False)["z"]))
    step = 1e-3 * float(np.sqrt(np.mean(x * x)))
    fd = np.zeros(n)
    for i in range(n):
        e = np.zeros(n)
        e[i] = step
        fd[i] = (8.0 * (loss(x + e) - loss(x - e)) - (loss(x + 2 * e) - loss(x - 2 * e))) / (12.0 * step)
    err = np.linalg.norm(got - fd) / np.linalg.norm(fd)
    print(f"order {order} even {even}: backward vs finite differences {err:.3e}")
    assert err < 1e-6


def test_order_one_is_the_ls_gain():
    x, y = pair()
    f = h.forward(x, y, 1, False, ridge=0.0, round32=False)
    g = np.dot(x, y) / np.dot(x, x)
    assert abs(f["c"][0] - g) <= 8 * 2.0 ** -53 * abs(g) * len(x) ** 0.5
    assert np.allclose(f["z"], g * x, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("order,even", [(5, False), (7, True)])
def test_scaling_invariances(order, even):
    x, y = pair()
    x, y = x.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)
    a = h.forward(x, y, order, even)
    b = h.forward(x, 0.25 * y, order, even)
    assert a["flag"] == b["flag"] == 0
    assert np.array_equal(b["c"], 0.25 * a["c"]) and np.array_equal(b["z"], 0.25 * a["z"]) and b["r"] == a["r"]
    c = h.forward(0.25 * x, 0.25 * y, order, even)
    assert np.array_equal(c["c"], a["c"]) and np.array_equal(c["z"], 0.25 * a["z"]) and c["r"] == 0.25 * a["r"]
    assert np.array_equal(c["sums"][1:-1], a["sums"][1:-1])


def rows(pk):
    r = np.random.default_rng(11)
    noise = r.standard_normal(N)
    w = r.standard_normal(N + 37)
    two = np.sin(2 * np.pi * 220.0 / 44100 * np.arange(N)) + 0.6 * np.sin(2 * np.pi * 3100.0 / 44100 * np.arange(N) + 1.0)
    return {k: v * (pk / np.max(np.abs(v))) for k, v in (("noise", noise), ("comb", w[37:] + 0.7 * w[:-37]), ("sines", two))}


@pytest.mark.parametrize("pk", [0.25, 1e-4])
def test_acceptance_rows(pk):
    """The issue's table: a cubic vanishes at order 3 (< 1e-6 of what the best gain leaves), the tanh comb row falls below 2e-2
    of it at odd order 5 (measured 2.8e-3), and an asymmetric curve needs the even powers."""
    for name, x in rows(pk).items():
        cubic = x - 0.3 * x ** 3 / pk ** 2
        assert h.esr(h.forward(x, cubic, 3, round32=False)["z"], cubic) < 1e-6 * h.ls_gain_esr(x, cubic), name
        asym = x - 0.2 * x ** 2 / pk - 0.15 * x ** 3 / pk ** 2
        assert h.esr(h.forward(x, asym, 3, False, round32=False)["z"], asym) > 0.5 * h.ls_gain_esr(x, asym), name
        assert h.esr(h.forward(x, asym, 3, True, round32=False)["z"], asym) < 1e-6 * h.ls_gain_esr(x, asym), name
    x = rows(pk)["comb"]
    soft = 0.25 * pk * np.tanh(2.0 * x / pk)
    ratio = h.esr(h.forward(x, soft, 5)["z"], soft) / h.ls_gain_esr(x, soft)
    print(f"tanh comb row at peak {pk}: shaped / gain-only ESR = {ratio:.3e}")
    assert ratio < 2e-2


def test_flags_on_hand_made_rows():
    x, y = pair(512)
    silent = h.forward(np.zeros(512), y, 5)
    assert silent["flag"] == 1 and silent["r"] == 1.0 and np.array_equal(silent["c"], [1.0, 0.0, 0.0])
    assert np.array_equal(silent["z"], np.zeros(512))
    # two distinct values +-1/2 in 1024 samples: r = 1/2, t = +-1, every moment is 1024 and sqrt(1024) = 32, so the factor is
    # exact, the Gram matrix has rank one and without a ridge the second pivot is exactly 0
    two = np.where(np.arange(1024) % 3 == 0, 0.5, -0.5)
    f = h.forward(two, np.tile(y, 2), 5, ridge=0.0)
    assert f["flag"] == 1 and f["r"] == 0.5 and f["pivots"] == [1024.0, 0.0]
    assert np.array_equal(f["z"], two)
    # a gain of 4 against max_gain 3
    g = h.forward(x, 4.0 * x, 3, max_gain=3.0)
    assert g["flag"] == 2 and np.array_equal(g["c"], [1.0, 0.0]) and np.array_equal(g["z"], x)
    assert h.forward(x, 4.0 * x, 3, max_gain=5.0)["flag"] == 0
    # a flagged row passes its gradient through unchanged
    dz = np.random.default_rng(0).standard_normal(512)
    assert np.array_equal(h.backward(dz, x, 4.0 * x, g, 3)["dy"], dz)

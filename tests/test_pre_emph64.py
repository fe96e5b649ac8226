"""CPU: the fp64 pre-emphasis reference of tests/helpers/pre_emph64.py -- the transpose identity, its explicit ESR gradient
against central finite differences at every sample, and the filter and loss values against the fixture recorded from the
real ``WrightPreEmph`` / ``WrightESRLoss`` / ``WrightDCLoss`` / ``ESRLoss`` (tests/golden/wright_pre_emph.npz).

Gates: <F u, v> = <u, F^T v> to 1e-12 (relative to the products' magnitude); finite differences to 1e-6 of max |gradient|
(the gate of the other fp64 adjoint tests: the loss is quadratic in y_hat, so a central difference is exact up to
rounding); the fixture to 1e-6 absolute (the reference runs in fp32 and sits within 1.6e-7 of fp64 on these inputs)."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import pre_emph64 as P

TAPS = {1: (1.0,), 2: (-0.95, 1.0), 3: (0.2, -0.9, 1.0)}
SHAPES = [(1, 2), (2, 9), (3, 67)]
GOLDEN_TAPS = [(-0.95, 1.0), (1.0,), (0.2, -0.9, 1.0)]
GOLDEN_SHAPES = [(2, 1), (257, 3), (4099, 2)]          # (T, B)


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("low_pass", [False, True])
@pytest.mark.parametrize("B,T", SHAPES)
def test_transpose_identity(K, low_pass, B, T):
    g = torch.Generator().manual_seed(100 * K + 10 * T + int(low_pass))
    L = T - 1 if low_pass else T
    u = torch.rand(B, T, generator=g, dtype=torch.float64) * 2 - 1
    v = torch.rand(B, L, generator=g, dtype=torch.float64) * 2 - 1
    lhs = (P.pre_emph64(u, TAPS[K], low_pass) * v).sum()
    rhs = (u * P.pre_emph_t64(v, TAPS[K], low_pass, T)).sum()
    scale = max(1.0, float((P.pre_emph64(u, TAPS[K], low_pass) * v).abs().sum()))
    err = abs(float(lhs - rhs)) / scale
    assert err < 1e-12, err


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("low_pass", [False, True])
@pytest.mark.parametrize("B,T", SHAPES)
def test_explicit_gradient_vs_central_differences(K, low_pass, B, T):
    g = torch.Generator().manual_seed(7 + 100 * K + 10 * T + int(low_pass))
    y = torch.rand(B, T, generator=g, dtype=torch.float64) * 1.6 - 0.8
    y_hat = 0.7 * y + 0.1 * (torch.rand(B, T, generator=g, dtype=torch.float64) - 0.5)
    w, eps = 0.75, 1e-8
    grad = P.esr_pre_grad64(y_hat, y, TAPS[K], low_pass, eps, w)
    fd = torch.empty_like(grad)
    h = 1e-3
    for b in range(B):
        for i in range(T):
            d = torch.zeros_like(y_hat)
            d[b, i] = h
            fd[b, i] = (P.esr_pre_value64(y_hat + d, y, TAPS[K], low_pass, eps, w)
                        - P.esr_pre_value64(y_hat - d, y, TAPS[K], low_pass, eps, w)) / (2 * h)
    err = float((grad - fd).abs().max() / grad.abs().max())
    assert err < 1e-6, err


def test_gradient_matches_autograd_of_the_value():
    y = torch.rand(3, 67, dtype=torch.float64) - 0.5
    y_hat = (0.5 * y).requires_grad_(True)
    P.esr_pre_value64(y_hat, y, TAPS[3], True, 1e-8, 1.3).backward()
    err = float((y_hat.grad - P.esr_pre_grad64(y_hat.detach(), y, TAPS[3], True, 1e-8, 1.3)).abs().max()
                / y_hat.grad.abs().max())
    assert err < 1e-12, err


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "wright_pre_emph.npz"))


def test_fixture_covers_the_stated_cases(golden):
    assert [tuple(float(np.float32(c)) for c in golden[f"taps_{i}"]) for i in range(3)] == \
        [tuple(float(np.float32(c)) for c in t) for t in GOLDEN_TAPS]
    for T, B in GOLDEN_SHAPES:
        assert golden[f"out_T{T}"].shape == (T, B, 1)
        for i in range(3):
            for lp in (0, 1):
                assert golden[f"f_out_T{T}_k{i}_lp{lp}"].shape == (T - lp, B, 1)
    assert not golden["tgt_T257"][:, 1].any() and not golden["tgt_T4099"][:, 1].any()      # the silent target rows


@pytest.mark.parametrize("T,B", GOLDEN_SHAPES)
@pytest.mark.parametrize("i", [0, 1, 2])
@pytest.mark.parametrize("lp", [0, 1])
def test_helper_reproduces_the_reference_fixture(golden, T, B, i, lp):
    taps = [float(c) for c in golden[f"taps_{i}"]]
    out = torch.from_numpy(golden[f"out_T{T}"])[:, :, 0].t()            # (B, T) rows
    tgt = torch.from_numpy(golden[f"tgt_T{T}"])[:, :, 0].t()
    key = f"T{T}_k{i}_lp{lp}"
    f_out, f_tgt = P.pre_emph64(out, taps, bool(lp)), P.pre_emph64(tgt, taps, bool(lp))
    err = float((f_out.t() - torch.from_numpy(golden["f_out_" + key])[:, :, 0].double()).abs().max())
    assert err < 1e-6, err
    err = float((f_tgt.t() - torch.from_numpy(golden["f_tgt_" + key])[:, :, 0].double()).abs().max())
    assert err < 1e-6, err
    # losses.py:34-38 on the filtered pair: per-clip ratio with eps 1e-8, mean over the clips
    esr = float(P.esr_pre_value64(out, tgt, taps, bool(lp), 1e-8))
    ref = float(golden["esr_" + key])
    assert abs(esr - ref) < 1e-6, (esr, ref)
    # wright_code.py:15-41 on the filtered pair (epsilon = 0.0: the ratios are batch-global, the silent row only adds 0)
    e = f_tgt - f_out
    energy = float((f_tgt * f_tgt).mean())
    w_esr = float((e * e).mean()) / energy
    w_dc = float(((f_tgt.mean(-1) - f_out.mean(-1)) ** 2).mean()) / energy
    assert abs(w_esr - float(golden["wesr_" + key])) < 1e-6, (w_esr, float(golden["wesr_" + key]))
    assert abs(w_dc - float(golden["wdc_" + key])) < 1e-6, (w_dc, float(golden["wdc_" + key]))

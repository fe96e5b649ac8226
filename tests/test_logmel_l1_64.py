"""CPU: the fp64 log-mel L1 reference (tests/helpers/logmel_l1_64.py: value and gradient by the explicit adjoint) against
torch autograd through an fp64 copy of oracle/losses.py:LogMelLoss (its window and filter bank rebuilt in fp64 from the
closed forms), at clip lengths that are and are not a multiple of the hop, for every n_fft the product supports.

Gates: value 1e-12 relative; gradient 1e-10 of max |g|.  The inputs include bands below eps in both signals (sgn(0) = 0:
no gradient) and bands below eps in the prediction only (the clamp passes no gradient there)."""
import ast
import os

import numpy as np
import pytest
import torch

from tests.helpers import fp64_refs as R
from tests.helpers.logmel_l1_64 import logmel_l1_64

HELPER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "logmel_l1_64.py")
CASES = [(T, n_fft) for T in (1024, 1000, 4500, 30000) for n_fft in (512, 1024, 2048) if T > n_fft // 2]


def test_helper_imports_only_numpy_scipy_and_the_fp64_primitives():
    tree = ast.parse(open(HELPER).read())
    mods = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            mods.update(a.name.split(".")[0] for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            mods.add(node.module)
    assert mods <= {"numpy", "scipy", "tests.helpers"}, mods


def _inputs(T, seed):
    g = np.random.default_rng(seed)
    n = np.arange(T) / 44100.0
    t = 0.3 * np.sin(2 * np.pi * 330.0 * n)[None, :] + g.uniform(-0.2, 0.2, (2, T))
    p = 0.8 * t + 0.1 * np.roll(t, 7, -1) + 0.05 * g.standard_normal((2, T))
    t[1, T // 3:T // 2] = 0.0                 # both silent over a span (row 1): bands below eps in both signals
    p[1, T // 3:T // 2] = 0.0
    p[0, T // 2:] *= 1e-6                     # a much quieter prediction (row 0): bands below eps in the prediction only
    return p[:, None, :], t[:, None, :]


def _oracle64(n_fft, hop, n_mels=256, sr=44100):
    from oracle import losses as olosses
    mod = olosses.LogMelLoss(sr, n_fft, hop, n_mels).double()
    with torch.no_grad():
        mod.spectrogram.spectrogram.window.copy_(torch.from_numpy(R.hann_periodic(n_fft)))
        mod.spectrogram.mel_scale.fb.copy_(torch.from_numpy(R.htk_fb64(n_fft, n_mels, sr)))
    return mod


@pytest.mark.parametrize("T,n_fft", CASES)
def test_logmel_l1_64_against_autograd(T, n_fft):
    hop = 256
    p, t = _inputs(T, T + n_fft)
    mod = _oracle64(n_fft, hop)
    xp = torch.from_numpy(p).requires_grad_(True)
    want = mod(xp, torch.from_numpy(t))
    want.backward()
    g_ref = xp.grad.numpy()
    val, g, (la, lb) = logmel_l1_64(p, t, n_fft, hop, 256)
    assert abs(val - float(want)) <= 1e-12 * abs(float(want)), (val, float(want))
    assert g.shape == p.shape
    e = float(np.abs(g - g_ref).max() / np.abs(g_ref).max())
    print(f"[measured] logmel_l1_64 vs autograd (T={T}, n_fft={n_fft}): value {abs(val - float(want)) / abs(float(want)):.1e}, "
          f"gradient {e:.1e} of max|g|")
    assert e <= 1e-10, e
    # the conventions the comparison pins are exercised (clips long enough for frames inside the quiet spans): ties (both
    # below eps) and prediction-only floors
    e_ = np.log(1e-7)
    assert np.any((la == e_) & (lb == e_))
    if T >= 4 * n_fft:
        assert np.any((la == e_) & (lb > e_))


def test_logmel_l1_64_fp32_yardstick_runs_in_fp32():
    p, t = _inputs(4500, 1)
    val, g, _ = logmel_l1_64(p.astype(np.float32), t.astype(np.float32), 1024, 256, 256, dtype=np.float32)
    val64, g64, _ = logmel_l1_64(p, t, 1024, 256, 256)
    assert g.dtype == np.float32
    assert abs(float(val) - val64) <= 1e-4 * val64
    assert 0.0 < float(np.abs(g - g64).max()) <= 1e-2 * float(np.abs(g64).max())


def test_radix2_yardstick_fft_is_the_dft():
    from tests.helpers.logmel_l1_64 import fft_radix2_c64
    g = np.random.default_rng(3)
    for n in (512, 1024, 2048):
        a = g.standard_normal((2, n))
        got = fft_radix2_c64(a.astype(np.float32))
        assert got.dtype == np.complex64
        want = np.fft.fft(a)
        e = float(np.abs(got - want).max() / np.abs(want).max())
        assert 0.0 < e <= 1e-5, (n, e)

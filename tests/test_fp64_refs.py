"""CPU: the independent fp64 references of tests/helpers/fp64_refs.py, checked against third-party definitions and known
values, and the product's filter bank / the C phaser oracle checked against them.

* the helper imports numpy, scipy and math only (no torch, no oracle, no product: it cannot share a formula with either)
* logmel64's framing, window and power against torch.stft in fp64 (centre, reflect pad): 1e-12
* MelSpectrogramHIP's fp32 HTK filter bank against the closed-form triangles: 1e-4 absolute (measured 5.8e-6 .. 4.5e-5,
  the fp32 evaluation of the slopes), support differing only where the fp64 value is below 1e-4 (measured 2.4e-14),
  partition of unity within 1e-6 between the first and the last band centre, the same empty bands
* the phaser's closed form: |A| = 1 on the unit circle, H(1) and H(-1) from the loop gain, a negligible tail
* orc_phaser (the arbiter of every other phaser test) at depth 0 against the closed form's impulse response
* mrstft64: its magnitudes against torch.stft in fp64 (centred short windows included), its value against the fp64
  evaluation of oracle/losses.py, its adjoint gradient against central finite differences, and the closed forms of
  x = a y and x = -y
"""
import ast
import itertools
import math
import os

import numpy as np
import pytest
import torch

from tests.helpers import fp64_refs as R

HELPER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "fp64_refs.py")


def test_helper_imports_only_numpy_scipy_math():
    tree = ast.parse(open(HELPER).read())
    roots = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            roots |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            assert node.level == 0, "relative import"
            roots.add(node.module.split(".")[0])
        elif isinstance(node, ast.Call) and getattr(node.func, "id", None) in ("__import__", "exec", "eval"):
            raise AssertionError("dynamic import / exec in the reference")
    assert roots <= {"numpy", "scipy", "math"}, roots


@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
def test_power_spectrum_matches_torch_stft_fp64(n_fft):
    g = np.random.default_rng(n_fft)
    for N, hop in [(n_fft // 2 + 1, 1), (n_fft // 2 + 1, 100), (n_fft + 1, 256), (5000, 256), (5000, 2 * n_fft)]:
        x = g.uniform(-1, 1, (2, N))
        P = R.power_spectrum(x, n_fft, hop)
        S = torch.stft(torch.from_numpy(x), n_fft, hop, window=torch.hann_window(n_fft, dtype=torch.float64),
                       center=True, pad_mode="reflect", return_complex=True)
        want = (S.abs() ** 2).transpose(-1, -2).numpy()
        assert P.shape == want.shape
        assert float(np.abs(P - want).max() / np.abs(want).max()) <= 1e-12
    # the Hann window is the periodic one, and torch's fp32 table (the product's buffer) is within 2.5e-7 of it
    assert np.abs(R.hann_periodic(n_fft) - torch.hann_window(n_fft, dtype=torch.float64).numpy()).max() <= 1e-15
    assert np.abs(R.hann_periodic(n_fft) - torch.hann_window(n_fft).double().numpy()).max() <= 2.5e-7


def test_logmel64_masks_clip_and_float32_yardstick():
    g = np.random.default_rng(5)
    x = g.uniform(-1, 1, (1, 4000))
    fb = R.htk_fb64(1024, 64, 44100)
    L, M = R.logmel64(x, 1024, 256, fb, 1e-7, (3, 7, 2, 5))
    assert L.shape == M.shape == (1, 64, 16)
    assert np.all(L[:, 3:7, :] == np.log(1e-7)) and np.all(L[:, :, 2:5] == np.log(1e-7))
    assert np.allclose(L[:, 10, 8], np.log(M[:, 10, 8]), rtol=0, atol=1e-15)
    L32, M32 = R.logmel64(x.astype(np.float32), 1024, 256, fb, 1e-7, dtype=np.float32)
    assert L32.dtype == np.float32
    assert float(np.abs(M32 - M).max() / M.max()) <= 1e-5


# the shapes of tests/test_gpu_edges.py::test_logmel_other_hops_rates_and_band_counts, and the shipped one
FB_SHAPES = [(1024, 256, 44100), (1024, 64, 44100), (1024, 96, 22050), (1024, 128, 48000), (512, 64, 44100),
             (2048, 128, 44100), (2048, 256, 44100), (512, 64, 16000), (2048, 512, 44100)]


@pytest.mark.parametrize("n_fft,n_mels,sr", FB_SHAPES)
def test_product_filter_bank_against_closed_form_triangles(n_fft, n_mels, sr):
    from mod_extraction_amd import models as am
    fb = am.MelSpectrogramHIP(sr, n_fft, 256, n_mels).mel_scale.fb.double().numpy()
    fb64 = R.htk_fb64(n_fft, n_mels, sr)
    assert fb.shape == fb64.shape == (n_fft // 2 + 1, n_mels)
    assert float(np.abs(fb - fb64).max()) <= 1e-4
    differ = (fb != 0) != (fb64 != 0)
    assert np.all(fb64[differ] < 1e-4)
    f_pts = R.mel_to_hz(np.linspace(0.0, float(R.hz_to_mel(sr // 2)), n_mels + 2))
    freqs = np.arange(n_fft // 2 + 1) * (sr // 2) / (n_fft // 2)
    inside = (freqs >= f_pts[1]) & (freqs <= f_pts[-2])
    assert float(np.abs(fb64[inside].sum(1) - 1).max()) <= 1e-12             # the triangles partition unity
    assert float(np.abs(fb[inside].sum(1) - 1).max()) <= 1e-6
    assert set(np.nonzero(~(fb != 0).any(0))[0]) == set(np.nonzero(~(fb64 != 0).any(0))[0])


def test_htk_mel_scale_known_values():
    # 1000 Hz = 1000 mel by construction of the scale; HTK's rounded constants (2595, 700) put it at 999.9855
    assert abs(float(R.hz_to_mel(1000.0)) - 999.9855) <= 1e-4
    assert abs(float(R.hz_to_mel(700.0)) - 2595.0 * math.log10(2.0)) <= 1e-9
    assert float(R.hz_to_mel(0.0)) == 0.0
    assert abs(float(R.mel_to_hz(R.hz_to_mel(12345.0))) - 12345.0) <= 1e-9
    fb = R.htk_fb64(1024, 256, 44100)
    assert int((fb.sum(0) == 0).sum()) == 20                                   # bands narrower than the bin spacing


@pytest.mark.parametrize("centre,feedback,mix,sr", [(440.0, 0.7, 1.0, 44100), (70.0, -0.7, 0.2, 48000),
                                                    (25000.0, 0.9, 1.0, 16000), (5.0, 0.35, 0.5, 44100)])
def test_phaser_closed_form_known_values(centre, feedback, mix, sr):
    z = np.exp(2j * math.pi * np.linspace(0.0, 0.5, 1001))
    a = R.allpass_coef(centre, sr)
    assert np.abs(np.abs(R.allpass_response(a, z)) - 1).max() <= 1e-12
    H1 = R.phaser_response(centre, feedback, mix, sr, np.array([1.0 + 0j]))[0]
    Hm1 = R.phaser_response(centre, feedback, mix, sr, np.array([-1.0 + 0j]))[0]
    assert abs(H1 - (mix / (1 + feedback) + 1 - mix)) <= 1e-12
    assert abs(Hm1 - (mix / (1 - feedback) + 1 - mix)) <= 1e-12
    h, tail = R.phaser_ir64(centre, feedback, mix, sr, 1 << 20)
    assert tail < 1e-12
    assert abs(h.sum() - H1.real) <= 1e-9                                      # DC gain = sum of the response
    assert R.phaser_cutoff(centre, sr) == min(max(centre, 20.0), min(20000.0, 0.49 * sr))


@pytest.mark.parametrize("sr", [44100, 48000, 16000])
def test_orc_phaser_depth0_against_closed_form(sr):
    """The C oracle at depth 0 against fftconvolve(x, h64) on the grid of tests/test_gpu_phaser_lti.py, 30 000 samples
    of 0.1-amplitude noise.  Gate: 2e-6 + 1.5 S, S = the closed form's own output change under a 1e-6 relative change
    of the cut-off.  The oracle's cut-off makes a round trip through fp32 log10 / pow (about one ulp of the exponent,
    1.1e-6 relative); measured max err / (2e-6 + S) = 0.67 over the grid (err 8e-8 at 440 Hz, 1e-4 at the upper clamp
    with feedback 0.9 and sr 16 kHz, where S is 1.5e-4)."""
    from scipy.signal import fftconvolve
    from oracle._cref import fptr, lib
    g = np.random.default_rng(sr)
    N = 30000
    for centre, fbk, mix in itertools.product((5.0, 20.0, 70.0, 440.0, 5000.0, 18000.0, 25000.0),
                                              (0.0, 0.35, 0.7, -0.7, 0.9), (0.2, 1.0)):
        x = (g.uniform(-1, 1, N) * 0.1).astype(np.float32)
        one = lambda v: np.full(1, v, np.float32)
        y = np.empty_like(x)
        lib().orc_phaser(fptr(x), fptr(one(1.0)), fptr(one(0.0)), fptr(one(centre)), fptr(one(fbk)), fptr(one(mix)),
                         1, N, float(sr), fptr(y), None)
        fc = R.phaser_cutoff(centre, sr)
        M = 1 << 18
        h, tail = R.phaser_ir64(fc, fbk, mix, sr, M)
        if tail >= 1e-9:                             # low cut-off, high feedback: the response is still ringing
            M = 1 << 20
            h, tail = R.phaser_ir64(fc, fbk, mix, sr, M)
        assert tail < 1e-9
        h2, _ = R.phaser_ir64(fc * (1 - 1e-6), fbk, mix, sr, M)
        y64 = fftconvolve(x.astype(np.float64), h[:N])[:N]
        S = float(np.abs(fftconvolve(x.astype(np.float64), h2[:N])[:N] - y64).max())
        err = float(np.abs(y - y64).max())
        assert err <= 2e-6 + 1.5 * S, (centre, fbk, mix, err, S)


# ---- MR-STFT loss -------------------------------------------------------------------------------------------------------
MR_DEFAULT = ((1024, 2048, 512), (120, 240, 50), (600, 1200, 240))


@pytest.mark.parametrize("n_fft,hop,win", [(1024, 120, 600), (2048, 240, 1200), (512, 50, 240), (512, 64, 301),
                                           (1024, 100, 1023)])
def test_mr_stft_magnitudes_match_torch_stft_fp64(n_fft, hop, win):
    """(512, 301) and (1024, 1023): windows shorter than n_fft by an odd amount (torch centres them at (n - win) // 2)."""
    g = np.random.default_rng(n_fft + win)
    x = g.uniform(-1, 1, (2, 5000))
    S = torch.stft(torch.from_numpy(x), n_fft, hop, win, torch.hann_window(win, dtype=torch.float64), center=True,
                   pad_mode="reflect", return_complex=True).transpose(-1, -2).numpy()
    X = R.stft(x, n_fft, hop, win)
    assert X.shape == S.shape
    assert float(np.abs(np.abs(X) - np.abs(S)).max() / np.abs(S).max()) <= 1e-12
    assert float(np.abs(X - S).max() / np.abs(S).max()) <= 1e-12


def _mr64(*cfg):
    """oracle/losses.py evaluated in fp64 (its fp32 window table replaced by torch's fp64 one)."""
    from oracle import losses as olosses

    class MR64(olosses.MultiResolutionSTFTLoss):
        def _mag(self, v, n_fft, hop, win):
            s = torch.stft(v.reshape(-1, v.size(-1)), n_fft, hop, win, torch.hann_window(win, dtype=torch.float64),
                           return_complex=True)
            return torch.sqrt(torch.clamp(s.real ** 2 + s.imag ** 2, min=self.eps))
    return MR64(*cfg)


@pytest.mark.parametrize("cfg", [MR_DEFAULT, ((512, 1024), (64, 100), (301, 1024))])
def test_mrstft64_value_matches_oracle_fp64(cfg):
    g = np.random.default_rng(7)
    y = g.uniform(-0.5, 0.5, (3, 7000))
    x = 0.7 * y + 0.2 * np.roll(y, 5, -1) + 0.05 * g.standard_normal(y.shape)
    x[1] *= 1e-3                                                  # a level mismatch: bins on both sides of the floor
    tot, terms, _ = R.mrstft64(x, y, *cfg)
    want = float(_mr64(*cfg)(torch.from_numpy(x), torch.from_numpy(y)))
    assert len(terms) == len(cfg[0])
    assert abs(float(tot) - want) <= 1e-12 * abs(want)
    assert abs(float(np.mean([sc + lm for sc, lm in terms])) - want) <= 1e-12 * abs(want)


def test_mrstft64_gradient_matches_central_differences():
    """40 sample positions: both reflect folds (the first and last n_fft/2 samples), around multiples of 32 hop (the
    kernel's runs of 32 frames) for each resolution, interior ones.  Step 1e-6 (measured 1.0e-7 of the largest tested
    gradient; 1e-5 and 1e-4 are worse: the curvature of the log term near weak bins).  The loss has kinks where a bin's
    |X| crosses |Y| (sign of the log term): T - 1024 of row 1 lies within 1e-6 of one and is not used."""
    T = 8000
    g = np.random.default_rng(3)
    y = g.uniform(-0.5, 0.5, (2, T))
    x = 0.7 * y + 0.2 * np.roll(y, 5, -1) + 0.05 * g.standard_normal((2, T))
    x[0, 2000:5000] *= 0.05
    for w_sc, w_log in ((1.0, 1.0), (0.3, 0.0), (0.0, 2.0)):
        _, _, dx = R.mrstft64(x, y, *MR_DEFAULT, w_sc=w_sc, w_log=w_log)
        pos = [(1, p) for p in (0, 1, 2, 7, 255, 511, 1023, T - 1, T - 2, T - 3, T - 256, T - 1000)]
        pos += [(r, p) for r, q in ((0, 32 * 50), (1, 64 * 50), (0, 96 * 50), (1, 128 * 50), (1, 32 * 120),
                                    (0, 64 * 120), (1, 32 * 240)) for p in (q - 1, q, q + 1)]
        pos += [(0, 2000), (0, 4999), (0, 3333), (1, 1234), (1, 4321), (0, 6789), (1, 2500)]
        assert len(pos) == 40
        h = 1e-6
        err = 0.0
        for r, p in pos:
            xp, xm = x.copy(), x.copy()
            xp[r, p] += h
            xm[r, p] -= h
            fd = (R.mrstft64(xp, y, *MR_DEFAULT, w_sc=w_sc, w_log=w_log)[0]
                  - R.mrstft64(xm, y, *MR_DEFAULT, w_sc=w_sc, w_log=w_log)[0]) / (2 * h)
            err = max(err, abs(fd - dx[r, p]))
        scale = max(abs(dx[r, p]) for r, p in pos)
        assert scale > 0
        assert err / scale <= 1e-6, (w_sc, w_log, err / scale)


@pytest.mark.parametrize("a", [0.5, 1.7, 0.1, 8.0])
def test_mrstft64_closed_form_scaled_and_negated(a):
    """x = a y with every bin of both above the floor: sc_r = |1 - a|, logmag_r = |ln a| exactly (to 1e-12).  x = -y:
    |X| = |Y| bit for bit (the transform of -y is the negated transform of y), so the loss and the gradient are exactly 0."""
    g = np.random.default_rng(11)
    T = 6000
    n = np.arange(T)
    y = 0.3 * np.sin(2 * math.pi * 0.01 * n)[None, :] + g.uniform(-0.3, 0.3, (2, T))
    x = a * y
    for (n_fft, hop, win) in zip(*MR_DEFAULT):
        P = np.abs(R.stft(y, n_fft, hop, win)) ** 2
        assert float(P.min()) * min(a, 1.0) ** 2 > 1e-8 * 1.01, (n_fft, float(P.min()))
    tot, terms, dx = R.mrstft64(x, y, *MR_DEFAULT)
    for sc, lm in terms:
        assert abs(sc - abs(1 - a)) <= 1e-12 * max(abs(1 - a), 1.0)
        assert abs(lm - abs(math.log(a))) <= 1e-12 * max(abs(math.log(a)), 1.0)
    assert abs(tot - (abs(1 - a) + abs(math.log(a)))) <= 1e-12 * (abs(1 - a) + abs(math.log(a)))
    tot, terms, dx = R.mrstft64(-y, y, *MR_DEFAULT)
    assert tot == 0.0 and all(sc == 0.0 and lm == 0.0 for sc, lm in terms)
    assert not np.any(dx)
    tot, terms, dx = R.mrstft64(-y.astype(np.float32), y.astype(np.float32), *MR_DEFAULT, dtype=np.float32)
    assert tot == 0.0 and not np.any(dx)


def test_mrstft64_float32_yardstick():
    """dtype float32: separate complex64 transforms, a plain fp32 evaluation close to fp64 at equal levels."""
    g = np.random.default_rng(2)
    y = g.uniform(-0.5, 0.5, (2, 8000))
    x = 0.8 * y + 0.05 * g.standard_normal(y.shape)
    t64, terms64, d64 = R.mrstft64(x, y, *MR_DEFAULT)
    t32, terms32, d32 = R.mrstft64(x.astype(np.float32), y.astype(np.float32), *MR_DEFAULT, dtype=np.float32)
    assert d32.dtype == np.float32 and isinstance(t32, np.float32)
    assert abs(float(t32) - t64) <= 1e-5 * t64
    assert float(np.abs(d32 - d64).max() / np.abs(d64).max()) <= 2e-3

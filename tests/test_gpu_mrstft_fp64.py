"""GPU: the MR-STFT loss (mx_mrstft_loss: mr_onepass_kernel with the gradient, mr_stats_kernel without) against an fp64
evaluation written from the definition (tests/helpers/fp64_refs.py: mrstft64 -- separate transforms of prediction and
target, the gradient by the explicit adjoint), at prediction / target levels that differ by up to 80 dB, over whole clips
and over spans inside a clip, and with each of the two terms alone.

The kernel packs the two real frames into ONE complex transform and separates the spectra by Hermitian symmetry; that
split leaves an error of the size of the louder frame on both spectra, so these are the inputs where it can go wrong.

Gates (per call):
  * the total and every per-resolution term of ``last_terms`` within 1e-5 (relative) of mrstft64
  * the gradient within max(2 x the yardstick's error, floor), in max-norm (floor 1e-4 of max |g64|) and in relative L2
    (floor 1e-5); the yardstick is mrstft64 run in fp32 (separate complex64 transforms): what a plain fp32 evaluation
    of the loss reaches on the same input
  * polarity-inverted frames (x = -y) have |X| = |Y| bit for bit in the reference: they contribute exactly 0

Measured on MI355X (gradient max-norm / relative L2 error against mrstft64): equal levels 3.7e-4 / 2.8e-4 (the fp32
conditioning of the log term; the yardstick is of the same size), prediction at 1e-2 / 1e-3 / 1e-4 of the target 1.4e-5 /
9.2e-7 / 1.8e-7 max-norm, target at 1e-2 / 1e-3 / 1e-4 of the prediction 4.2e-5 / 1.9e-6 / 4.3e-7, the 1e-4 span 2.5e-6,
the polarity span 1.0e-4; every value and term within 1e-6 relative.  Before the kernel equalised the packed levels, the
prediction-quieter cases failed by 12x (1e-2) to 240x (the 1e-4 span) in max-norm, the polarity-inverted clip gave a loss of
2.4e-7 instead of 0, and the polarity span 8.8e-2 (random-sign log terms of rounding-level bin differences).
"""
import numpy as np
import pytest
import torch

from tests.helpers import fp64_refs as R

pytestmark = pytest.mark.gpu

DEFAULT = ((1024, 2048, 512), (120, 240, 50), (600, 1200, 240))
B, T = 2, 12000
# spans of at least two runs of 32 frames of the 512-point resolution (2 x 32 x 50 = 3200 samples), one per row
SPANS = ((3000, 7000), (5000, 9500))
# polarity spans: long enough that some samples are reached only by frames inside the span (the 2048-point frames too)
NEG_SPANS = ((2000, 10000), (1500, 9000))


def pair(seed=0):
    """(prediction, target) (B, T) float64 at about 0.5 peak: a sine and noise, and a detuned, delayed, noisier copy."""
    g = np.random.default_rng(seed)
    n = np.arange(T) / 44100.0
    t = 0.3 * np.sin(2 * np.pi * 330.0 * n)[None, :] + g.uniform(-0.2, 0.2, (B, T))
    p = 0.8 * t + 0.1 * np.roll(t, 7, -1) + 0.05 * g.standard_normal((B, T))
    return p, t


def kernel(dev, x, y, cfg=DEFAULT, w_sc=1.0, w_log=1.0):
    """Value, last_terms and gradient through the module (autograd.Function, forward + backward)."""
    from mod_extraction_amd import mrstft as amr
    mod = amr.MultiResolutionSTFTLoss(*cfg, w_sc=w_sc, w_log_mag=w_log)
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev).requires_grad_(True)
    loss = mod(xd, torch.from_numpy(np.ascontiguousarray(y, np.float32)).to(dev))
    loss.backward()
    return float(loss), mod.last_terms.cpu().double().numpy(), xd.grad.cpu().double().numpy()


def check(dev, x, y, tag, cfg=DEFAULT, w_sc=1.0, w_log=1.0):
    x, y = x.astype(np.float32), y.astype(np.float32)
    val, terms, g = kernel(dev, x, y, cfg, w_sc, w_log)
    t64, terms64, g64 = R.mrstft64(x.astype(np.float64), y.astype(np.float64), *cfg, w_sc=w_sc, w_log=w_log)
    _, _, g32 = R.mrstft64(x, y, *cfg, w_sc=w_sc, w_log=w_log, dtype=np.float32)
    want = [float(v) for sc, lm in terms64 for v in (sc, lm)] + [float(t64)]
    assert len(terms) == len(want)
    assert abs(val - t64) <= 1e-5 * abs(t64), (tag, val, t64)
    for i, (got, w) in enumerate(zip(terms, want)):
        assert abs(got - w) <= 1e-5 * abs(w), (tag, i, got, w)
    scale, l2 = float(np.abs(g64).max()), float(np.linalg.norm(g64))
    assert scale > 0
    e_max = float(np.abs(g - g64).max()) / scale
    y_max = float(np.abs(g32 - g64).max()) / scale
    e_l2 = float(np.linalg.norm(g - g64)) / l2
    y_l2 = float(np.linalg.norm(g32 - g64)) / l2
    assert e_max <= max(2.0 * y_max, 1e-4), (tag, e_max, y_max)
    assert e_l2 <= max(2.0 * y_l2, 1e-5), (tag, e_l2, y_l2)
    return g, g64


@pytest.mark.parametrize("ratio", [1.0, 1e-2, 1e-3, 1e-4, 1e2, 1e3, 1e4])
def test_mrstft_level_grid(dev, ratio):
    """Prediction / target level ratio over whole clips: the louder signal at about 0.5, the other scaled down."""
    p, t = pair(1)
    x, y = (ratio * p, t) if ratio <= 1 else (p, t / ratio)
    check(dev, x, y, ratio)


def _lsb_noise(g, n):
    return g.integers(-1, 2, n) / 32768.0                  # -1, 0, +1 LSB of 16-bit audio


@pytest.mark.parametrize("case", ["pred_1e-4", "target_lsb_noise", "pred_zeros", "target_zeros"])
def test_mrstft_level_mismatch_inside_a_clip(dev, case):
    p, t = pair(2)
    g = np.random.default_rng(3)
    for r, (s0, s1) in enumerate(SPANS):
        if case == "pred_1e-4":
            p[r, s0:s1] *= 1e-4
        elif case == "target_lsb_noise":
            t[r, s0:s1] = _lsb_noise(g, s1 - s0)
        elif case == "pred_zeros":
            p[r, s0:s1] = 0.0
        else:
            t[r, s0:s1] = 0.0
    check(dev, p, t, case)


def test_mrstft_polarity_inverted_clip(dev):
    """x = -y: |X| = |Y| bin for bin in the reference, so the loss and the gradient are exactly 0 (as for x == y)."""
    _, t = pair(4)
    t = t.astype(np.float32)
    tot, terms, g64 = R.mrstft64(-t.astype(np.float64), t.astype(np.float64), *DEFAULT)
    assert tot == 0.0 and not np.any(g64)
    val, terms, g = kernel(dev, -t, t)
    assert val == 0.0
    assert not np.any(terms)
    assert float(np.abs(g).max()) == 0.0


def exact_zero_region(span, cfg=DEFAULT):
    """Samples every frame of which (at every resolution) lies inside the span together with its two neighbours (frames
    are transformed and overlap-added in pairs)."""
    s0, s1 = span
    ok = np.ones(T, bool)
    for n_fft, hop, _ in zip(*cfg):
        nf = T // hop + 1
        inside = np.array([f * hop - n_fft // 2 >= s0 and f * hop + n_fft // 2 <= s1 for f in range(nf)])
        good = inside & np.r_[False, inside[:-1]] & np.r_[inside[1:], False]
        for f in np.nonzero(~good)[0]:
            ok[max(f * hop - n_fft // 2, 0):max(min(f * hop + n_fft // 2, T), 0)] = False
    return ok


def test_mrstft_polarity_inverted_span(dev):
    """x = -y over a span of each clip: the whole clip against the reference, and the samples that only the span's
    frames reach receive exactly 0 -- in the reference and in the kernel."""
    p, t = pair(5)
    for r, (s0, s1) in enumerate(NEG_SPANS):
        p[r, s0:s1] = -t[r, s0:s1].astype(np.float32)
    g, g64 = check(dev, p, t, "neg_span")
    for r, span in enumerate(NEG_SPANS):
        zone = exact_zero_region(span)
        assert zone.sum() >= 1000
        assert not np.any(g64[r, zone])
        assert float(np.abs(g[r, zone]).max()) == 0.0, r


@pytest.mark.parametrize("w_sc,w_log", [(1.0, 0.0), (0.0, 1.0)])
@pytest.mark.parametrize("ratio", [1.0, 1e-3, 1e3])
def test_mrstft_terms_separately(dev, w_sc, w_log, ratio):
    """Each term alone: the gradient of the spectral convergence alone is well conditioned (no 1 / |X|)."""
    p, t = pair(6)
    x, y = (ratio * p, t) if ratio <= 1 else (p, t / ratio)
    check(dev, x, y, (w_sc, w_log, ratio), w_sc=w_sc, w_log=w_log)


def _rows(dev, x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)


def test_mrstft_value_only_path_matches_gradient_path(dev):
    """need_grad=False runs mr_stats_kernel instead of the one-pass kernel: same value and terms to 1e-6."""
    from mod_extraction_amd import mrstft as amr
    p, t = pair(7)
    for x, y in ((p, t), (1e-3 * p, t), (p, 1e-3 * t)):
        mod = amr.MultiResolutionSTFTLoss()
        a, b = _rows(dev, x), _rows(dev, y)
        v1, dx = amr.mrstft_value_and_grad(mod, a, b, need_grad=True)
        terms1 = mod.last_terms.cpu().double().numpy()
        v0, none = amr.mrstft_value_and_grad(mod, a, b, need_grad=False)
        terms0 = mod.last_terms.cpu().double().numpy()
        assert none is None and dx is not None
        assert float(np.abs(terms0 - terms1).max() / np.abs(terms1).max()) <= 1e-6
        assert abs(float(v0) - float(v1)) <= 1e-6 * abs(float(v1))


def test_mrstft_scale_scales_value_and_gradient(dev):
    from mod_extraction_amd import mrstft as amr
    p, t = pair(8)
    mod = amr.MultiResolutionSTFTLoss()
    a, b = _rows(dev, p), _rows(dev, t)
    v1, g1 = amr.mrstft_value_and_grad(mod, a, b)
    terms1 = mod.last_terms.clone()
    vs, gs = amr.mrstft_value_and_grad(mod, a, b, scale=0.37)
    terms_s = mod.last_terms.clone()
    assert abs(float(vs) - 0.37 * float(v1)) <= 1e-6 * abs(float(v1))
    assert torch.equal(terms_s[:-1], terms1[:-1])                      # the per-resolution terms are unscaled
    g1, gs = g1.cpu().double(), gs.cpu().double()
    assert float((gs - 0.37 * g1).abs().max() / (0.37 * g1.abs().max())) <= 1e-6


def test_mrstft_strided_rows_bit_identical(dev):
    """Rows of (B, T) views into (B, T + 37) buffers (odd row stride) give what contiguous copies give, bit for bit."""
    from mod_extraction_amd import mrstft as amr
    p, t = pair(9)
    bufx = torch.zeros((B, T + 37), device=dev)
    bufy = torch.zeros((B, T + 37), device=dev)
    bufx[:, 5:5 + T] = _rows(dev, p)
    bufy[:, 11:11 + T] = _rows(dev, t)
    xv, yv = bufx[:, 5:5 + T], bufy[:, 11:11 + T]
    assert xv.stride() == (T + 37, 1) and not xv.is_contiguous()
    mod = amr.MultiResolutionSTFTLoss()
    v_s, g_s = amr.mrstft_value_and_grad(mod, xv, yv)
    terms_s = mod.last_terms.clone()
    v_c, g_c = amr.mrstft_value_and_grad(mod, xv.contiguous(), yv.contiguous())
    assert torch.equal(mod.last_terms, terms_s) and torch.equal(v_s, v_c)
    assert torch.equal(g_s, g_c)
    v0, _ = amr.mrstft_value_and_grad(mod, xv, yv, need_grad=False)
    terms0 = mod.last_terms.clone()
    amr.mrstft_value_and_grad(mod, xv.contiguous(), yv.contiguous(), need_grad=False)
    assert torch.equal(mod.last_terms, terms0)

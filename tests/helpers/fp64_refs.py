"""Independent fp64 references for the mel front end and the phaser (TEST INFRASTRUCTURE ONLY).

Everything here is written from the definitions of the operations, not from the product or the oracle: this module
imports numpy, scipy and math only (tests/test_fp64_refs.py checks that), so a formula shared by the product and the
oracle cannot hide in both sides of a comparison.

* ``htk_fb64``      the HTK triangular mel filter bank, one triangle per band from its three mel points.
* ``logmel64``      centre/reflect pad -> periodic Hann -> rfft -> |X|^2 -> @ fb -> masks -> clip -> log.
                    ``dtype=numpy.float32`` runs the same pipeline in fp32 (scipy.fft): the yardstick of how large a
                    plain fp32 evaluation's error is.
* ``phaser_ir64``   the phaser at depth 0 (a constant cut-off, so an LTI system) as a closed-form transfer function,
                    turned into an impulse response on an M-point frequency grid.
"""
import math

import numpy as np
import scipy.fft


def hz_to_mel(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_to_hz(m):
    return 700.0 * (10.0 ** (np.asarray(m, dtype=np.float64) / 2595.0) - 1.0)


def htk_fb64(n_fft: int, n_mels: int, sr: int) -> np.ndarray:
    """(n_fft/2 + 1, n_mels) fp64: band m is the triangle through the mel points m, m+1, m+2 of n_mels + 2 points equally
    spaced on the HTK mel scale between 0 Hz and sr//2; bin k sits at k * (sr//2) / (n_fft/2) Hz."""
    n_bins = n_fft // 2 + 1
    f_max = float(sr // 2)
    freqs = np.arange(n_bins, dtype=np.float64) * (f_max / (n_fft // 2))
    m_pts = np.linspace(0.0, float(hz_to_mel(f_max)), n_mels + 2)
    f_pts = mel_to_hz(m_pts)
    fb = np.zeros((n_bins, n_mels), dtype=np.float64)
    for m in range(n_mels):
        f_l, f_c, f_r = f_pts[m], f_pts[m + 1], f_pts[m + 2]
        rise = (freqs - f_l) / (f_c - f_l)
        fall = (f_r - freqs) / (f_r - f_c)
        fb[:, m] = np.maximum(0.0, np.minimum(rise, fall))
    return fb


def hann_periodic(n_fft: int, dtype=np.float64) -> np.ndarray:
    n = np.arange(n_fft, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * math.pi * n / n_fft)).astype(dtype)


def frames_reflect(x: np.ndarray, n_fft: int, hop: int, n_frames: int) -> np.ndarray:
    """(..., N) -> (..., n_frames, n_fft): frame t holds padded samples [t*hop, t*hop + n_fft) of x reflect-padded by
    n_fft/2 on both sides (the edge sample is not repeated)."""
    N = x.shape[-1]
    half = n_fft // 2
    if N <= half:
        raise ValueError("reflect padding needs more than n_fft/2 samples")
    if n_frames > N // hop + 1:
        raise ValueError("frames beyond the padded clip")
    i = np.arange(n_frames)[:, None] * hop + np.arange(n_fft)[None, :] - half
    i = np.where(i < 0, -i, i)
    i = np.where(i >= N, 2 * (N - 1) - i, i)
    return x[..., i]


def power_spectrum(x: np.ndarray, n_fft: int, hop: int, n_frames: int = None, dtype=np.float64,
                   window=None) -> np.ndarray:
    """(..., N) -> (..., n_frames, n_fft/2 + 1) = |rfft(window * frame)|^2; window: the periodic Hann window unless a
    table of n_fft values is given."""
    x = np.asarray(x)
    if n_frames is None:
        n_frames = x.shape[-1] // hop + 1
    w = hann_periodic(n_fft, dtype) if window is None else np.asarray(window, dtype=dtype)
    fr = frames_reflect(x.astype(dtype), n_fft, hop, n_frames) * w
    if dtype == np.float64:
        X = np.fft.rfft(fr, axis=-1)
    else:
        X = scipy.fft.rfft(fr, axis=-1)                 # complex64 in, complex64 out
    return np.ascontiguousarray(X.real * X.real + X.imag * X.imag, dtype=dtype)     # (C order: a fast `@ fb`)


def logmel64(x, n_fft: int, hop: int, fb, eps: float, masks=(0, 0, 0, 0), n_frames: int = None, dtype=np.float64,
             window=None):
    """x (..., N) -> (log_mel, mel), both (..., n_mels, n_frames): mel = power @ fb (no masks), log_mel =
    log(max(mel with band rows [f0, f1) and frames [t0, t1) set to 0, eps))."""
    fb = np.asarray(fb, dtype=dtype)
    P = power_spectrum(x, n_fft, hop, n_frames, dtype, window)
    mel = np.swapaxes(P @ fb, -1, -2)
    f0, f1, t0, t1 = (int(v) for v in masks)
    masked = mel.copy()
    masked[..., f0:f1, :] = 0
    masked[..., :, t0:t1] = 0
    return np.log(np.maximum(masked, dtype(eps))), mel


# ---- phaser at depth 0 -------------------------------------------------------------------------------------------------
def phaser_cutoff(centre: float, sr: float) -> float:
    return min(max(float(centre), 20.0), min(20000.0, 0.49 * sr))


def allpass_coef(centre: float, sr: float) -> float:
    g = math.tan(math.pi * phaser_cutoff(centre, sr) / sr)
    return (g - 1.0) / (g + 1.0)


def allpass_response(a: float, z: np.ndarray) -> np.ndarray:
    """A(z) = (a + z^-1) / (1 + a z^-1): one first-order all-pass stage."""
    zi = 1.0 / z
    return (a + zi) / (1.0 + a * zi)


def phaser_response(centre: float, feedback: float, mix: float, sr: float, z: np.ndarray) -> np.ndarray:
    """H(z) = mix * A^6 / (1 + fb z^-1 A^6) + (1 - mix): six stages in a loop that feeds the previous output back
    (subtracted, scaled by fb), linear dry/wet mix."""
    A6 = allpass_response(allpass_coef(centre, sr), z) ** 6
    return mix * A6 / (1.0 + feedback / z * A6) + (1.0 - mix)


def phaser_ir64(centre: float, feedback: float, mix: float, sr: float, M: int = 1 << 20):
    """(h, tail): the impulse response h[0..M) of H sampled on the M-point grid z = exp(2 pi i k / M) (irfft), and
    max|h| over its last M/8 samples -- time aliasing of the infinite response is below that."""
    z = np.exp(2j * math.pi * np.arange(M // 2 + 1) / M)
    h = np.fft.irfft(phaser_response(centre, feedback, mix, sr, z), n=M)
    return h, float(np.abs(h[-(M // 8):]).max())

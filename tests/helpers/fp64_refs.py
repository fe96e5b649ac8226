"""Independent fp64 references for the mel front end, the phaser and the MR-STFT loss (TEST INFRASTRUCTURE ONLY).

Everything here is written from the definitions of the operations, not from the product or the oracle: this module
imports numpy, scipy and math only (tests/test_fp64_refs.py checks that), so a formula shared by the product and the
oracle cannot hide in both sides of a comparison.

* ``htk_fb64``      the HTK triangular mel filter bank, one triangle per band from its three mel points.
* ``logmel64``      centre/reflect pad -> periodic Hann -> rfft -> |X|^2 -> @ fb -> masks -> clip -> log.
                    ``dtype=numpy.float32`` runs the same pipeline in fp32 (scipy.fft): the yardstick of how large a
                    plain fp32 evaluation's error is.
* ``mrstft64``      the multi-resolution STFT loss (auraloss definition: spectral convergence + log-magnitude L1, mean over
                    resolutions), its per-resolution terms, and d total / d x by the explicit adjoint (inverse transform
                    of the per-bin gradient, window, overlap-add, reflect fold) -- no autograd.  ``dtype=numpy.float32``
                    runs it on SEPARATE complex64 transforms: the fp32 yardstick.
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


# ---- multi-resolution STFT loss ----------------------------------------------------------------------------------------
def mr_window(n_fft: int, win_length: int, dtype=np.float64) -> np.ndarray:
    """The periodic Hann window of win_length placed in an n_fft frame at offset (n_fft - win_length) // 2, zeros around."""
    w = np.zeros(n_fft, dtype=np.float64)
    left = (n_fft - win_length) // 2
    w[left:left + win_length] = hann_periodic(win_length)
    return w.astype(dtype)


def stft(x, n_fft: int, hop: int, win_length: int, dtype=np.float64) -> np.ndarray:
    """(..., N) -> (..., 1 + N // hop, n_fft/2 + 1) complex: rfft of every centre / reflect-padded frame times mr_window.
    dtype float32: scipy.fft on float32 frames (complex64 out)."""
    x = np.asarray(x).astype(dtype)
    fr = frames_reflect(x, n_fft, hop, x.shape[-1] // hop + 1) * mr_window(n_fft, win_length, dtype)
    return np.fft.rfft(fr, axis=-1) if dtype == np.float64 else scipy.fft.rfft(fr, axis=-1)


def mrstft64(x, y, fft_sizes, hops, win_lengths, eps=1e-8, w_sc=1.0, w_log=1.0, dtype=np.float64):
    """x (prediction), y (target): (..., N).  Returns (total, [(sc_r, logmag_r) per resolution], d total / d x).

    Per resolution: mag = sqrt(max(|X|^2, eps)) over every bin of every frame of the whole batch,
    sc = ||Ym - Xm||_F / ||Ym||_F, logmag = mean |log Xm - log Ym|;  total = mean_r (w_sc sc_r + w_log logmag_r).
    Gradient: per bin G = dL/d|X| * X / |X| (0 where |X|^2 <= eps; sign(0) = 0; the sc part 0 when ||Ym - Xm|| = 0), per
    frame n_fft * Re(ifft(G zero-extended to n_fft bins)) times the window, overlap-added into the padded signal, whose
    reflect padding is then folded back onto the clip.  X and Y come from separate transforms in either dtype."""
    x = np.asarray(x).astype(dtype)
    y = np.asarray(y).astype(dtype)
    assert x.shape == y.shape
    shape, N = x.shape, x.shape[-1]
    x, y = x.reshape(-1, N), y.reshape(-1, N)
    B = x.shape[0]
    n_res = len(fft_sizes)
    eps_t = dtype(eps)
    total = dtype(0.0)
    terms = []
    dx = np.zeros((B, N), dtype=dtype)
    for n_fft, hop, wl in zip(fft_sizes, hops, win_lengths):
        half = n_fft // 2
        n_frames = N // hop + 1
        X = stft(x, n_fft, hop, wl, dtype)
        Y = stft(y, n_fft, hop, wl, dtype)
        px = X.real * X.real + X.imag * X.imag
        py = Y.real * Y.real + Y.imag * Y.imag
        xm = np.sqrt(np.maximum(px, eps_t))
        ym = np.sqrt(np.maximum(py, eps_t))
        nd = np.sqrt(np.sum((ym - xm) ** 2))
        ny = np.sqrt(np.sum(ym ** 2))
        sc = nd / ny
        ld = np.log(xm) - np.log(ym)
        lm = np.mean(np.abs(ld))
        terms.append((sc, lm))
        total = total + dtype(w_sc) * sc + dtype(w_log) * lm
        # d total / d |X| per bin, then G = that * X / |X| on the bins above the floor
        alpha = dtype(w_sc) / (dtype(n_res) * nd * ny) if nd > 0 else dtype(0.0)
        c_log = dtype(w_log) / (dtype(n_res) * dtype(ld.size))
        dm = alpha * (xm - ym) + c_log * np.sign(ld) / xm
        G = np.where(px > eps_t, dm / xm, dtype(0.0)) * X
        Gext = np.zeros(G.shape[:-1] + (n_fft,), dtype=G.dtype)
        Gext[..., :half + 1] = G
        ifft = np.fft.ifft if dtype == np.float64 else scipy.fft.ifft
        gf = dtype(n_fft) * ifft(Gext, axis=-1).real.astype(dtype) * mr_window(n_fft, wl, dtype)    # (B, frames, n_fft)
        # overlap-add into the padded signal (padded position p = sample p - n_fft/2)
        P = (n_frames - 1) * hop + n_fft
        pos = (np.arange(n_frames)[:, None] * hop + np.arange(n_fft)[None, :]).ravel()
        rows = np.arange(B)[:, None] * P
        padded = np.bincount((rows + pos[None, :]).ravel(), weights=gf.reshape(B, -1).ravel().astype(np.float64),
                             minlength=B * P).astype(dtype).reshape(B, P)
        # fold the reflect padding back: padded position p holds sample reflect(p - n_fft/2)
        s = np.arange(P) - half
        s = np.where(s < 0, -s, s)
        s = np.where(s >= N, 2 * (N - 1) - s, s)
        dx += np.bincount((np.arange(B)[:, None] * N + s[None, :]).ravel(), weights=padded.ravel().astype(np.float64),
                          minlength=B * N).astype(dtype).reshape(B, N)
    return total / dtype(n_res), terms, dx.reshape(shape)

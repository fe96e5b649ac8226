"""Independent fp64 reference of the log-mel L1 loss and its gradient (TEST INFRASTRUCTURE ONLY).

Written from the definition (mod_extraction/losses.py:105-130: torchaudio MelSpectrogram -- centre / reflect padding of
n_fft/2, periodic Hann, power 2, HTK filter bank, no norm -- then mean |log max(mel(x), eps) - log max(mel(y), eps)|), with
numpy, scipy and the primitives of fp64_refs.py only (no torch, no oracle, no product).  The gradient is the explicit
adjoint, no autograd:  dM = sgn(la - lb) [M_x >= eps] / (M_x count),  dP = dM @ fb^T,  dX = 2 dP X  ->  n_fft Re ifft of the
zero-extended one-sided spectrum -> window -> overlap-add by hop -> fold of the reflect padding onto the clip.
``dtype=numpy.float32`` runs the same pipeline in fp32 (separate transforms of prediction and target): the yardstick of what
a plain fp32 evaluation reaches.  Its forward transform is scipy.fft's real FFT (``fft="scipy"``) or a textbook iterative
radix-2 complex FFT of the real frame in complex64 (``fft="radix2"``): the gradient of a weak band divides by the band's
power, so the two plain fp32 transforms can differ by 10x there (measured: a weak bin of an even-symmetric, reflect-padded
first frame) -- a yardstick should not be one lucky rounding.
"""
import numpy as np
import scipy.fft

from tests.helpers import fp64_refs as R


def fft_radix2_c64(a: np.ndarray) -> np.ndarray:
    """Complex DFT along the last axis (power-of-two length) by iterative radix-2 decimation in time, every operation in
    complex64, twiddles exp(-i pi j / m) rounded to complex64."""
    x = np.asarray(a).astype(np.complex64)
    n = x.shape[-1]
    bits = n.bit_length() - 1
    assert 1 << bits == n
    idx = np.arange(n)
    rev = np.zeros(n, dtype=np.int64)
    for b in range(bits):
        rev |= ((idx >> b) & 1) << (bits - 1 - b)
    x = x[..., rev]
    m = 1
    while m < n:
        w = np.exp(-1j * np.pi * np.arange(m) / m).astype(np.complex64)
        x = x.reshape(x.shape[:-1] + (n // (2 * m), 2, m))
        t = x[..., 1, :] * w
        u = x[..., 0, :]
        x = np.stack([u + t, u - t], axis=-2).reshape(x.shape[:-3] + (n,))
        m *= 2
    return x


def logmel_l1_64(x, y, n_fft: int, hop: int, n_mels: int, sr: int = 44100, eps: float = 1e-7, fb=None, window=None,
                 dtype=np.float64, fft: str = "scipy"):
    """x (prediction), y (target): (..., N).  Returns (value, d value / d x with x's shape, (la, lb) as (rows, frames,
    n_mels)).  fb: (n_fft/2 + 1, n_mels) bank (default: htk_fb64); window: n_fft values (default: the periodic Hann);
    fft: the fp32 forward transform, "scipy" or "radix2" (fp64 always uses numpy.fft)."""
    x = np.asarray(x).astype(dtype)
    y = np.asarray(y).astype(dtype)
    assert x.shape == y.shape
    shape, N = x.shape, x.shape[-1]
    x, y = x.reshape(-1, N), y.reshape(-1, N)
    B = x.shape[0]
    half = n_fft // 2
    n_frames = N // hop + 1
    fb = np.asarray(R.htk_fb64(n_fft, n_mels, sr) if fb is None else fb, dtype=dtype)
    w = R.hann_periodic(n_fft, dtype) if window is None else np.asarray(window, dtype=dtype)
    if dtype == np.float64:
        rfft = np.fft.rfft
    elif fft == "radix2":
        rfft = lambda a, axis: fft_radix2_c64(a)[..., :half + 1]      # noqa: E731
    else:
        rfft = scipy.fft.rfft
    X = rfft(R.frames_reflect(x, n_fft, hop, n_frames) * w, axis=-1)          # (B, frames, n_fft/2 + 1)
    Y = rfft(R.frames_reflect(y, n_fft, hop, n_frames) * w, axis=-1)
    px = (X.real * X.real + X.imag * X.imag).astype(dtype)
    py = (Y.real * Y.real + Y.imag * Y.imag).astype(dtype)
    mx, my = px @ fb, py @ fb                                                # (B, frames, n_mels)
    e = dtype(eps)
    la, lb = np.log(np.maximum(mx, e)), np.log(np.maximum(my, e))
    d = la - lb
    value = np.mean(np.abs(d))
    # torch's conventions: sgn(0) = 0; clamp(min=eps) passes the gradient where its input >= eps
    live = mx >= e
    dm = np.where(live, np.sign(d) / np.where(live, mx, dtype(1.0)), dtype(0.0)) / dtype(d.size)
    dp = dm @ fb.T                                                           # (B, frames, n_fft/2 + 1)
    G = dtype(2.0) * dp * X
    Gext = np.zeros(G.shape[:-1] + (n_fft,), dtype=G.dtype)
    Gext[..., :half + 1] = G
    ifft = np.fft.ifft if dtype == np.float64 else scipy.fft.ifft
    gf = dtype(n_fft) * ifft(Gext, axis=-1).real.astype(dtype) * w          # (B, frames, n_fft)
    # overlap-add into the padded signal (padded position p = sample p - n_fft/2), then fold the reflect padding back
    P = (n_frames - 1) * hop + n_fft
    pos = (np.arange(n_frames)[:, None] * hop + np.arange(n_fft)[None, :]).ravel()
    padded = np.bincount((np.arange(B)[:, None] * P + pos[None, :]).ravel(), weights=gf.reshape(B, -1).ravel().astype(np.float64),
                         minlength=B * P).astype(dtype).reshape(B, P)
    s = np.arange(P) - half
    s = np.where(s < 0, -s, s)
    s = np.where(s >= N, 2 * (N - 1) - s, s)
    dx = np.bincount((np.arange(B)[:, None] * N + s[None, :]).ravel(), weights=padded.ravel().astype(np.float64),
                     minlength=B * N).astype(dtype).reshape(B, N)
    return value, dx.reshape(shape), (la, lb)

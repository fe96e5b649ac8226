"""The harness of the kernel-level GPU unit tests (tests/test_gpu_block1_units.py, tests/test_gpu_midblock_units.py): every
output lives between two guard bands pre-filled with a NaN bit pattern that must survive, the pad columns of fp32 inputs hold
1e30, entry points are called through ``call`` (a non-zero status raises) or ``status`` (returns it), and every tolerance gate
is ``ratio(...) <= tol``: the worst |got - ref| / bound."""
import numpy as np
import torch

GUARD = 64                                   # 4-byte words on each side of every output
SENT = 0x7FC5A5A5                            # a quiet NaN with a payload: no kernel here produces it
U = 2.0 ** -23
POISON = np.float32(1.0e30)                  # pad columns of inputs: must never reach a result
f16, f32, f64 = np.float16, np.float32, np.float64
ARG, UNSUPPORTED = -1, -2


def _hip():
    from mod_extraction_amd import _hip as h
    return h


class Out:
    """A device output of n elements of ``dtype`` (float32 / uint32 / float16 / uint8) between guard bands; body and guards are
    pre-filled with the sentinel words (``init``: the body's initial content).  Kept on the device: the large planes are
    compared there."""

    def __init__(self, dev, n, dtype=f32, init=None):
        self.n, self.dtype = int(n), np.dtype(dtype)
        self.per = 4 // self.dtype.itemsize                              # elements per 4-byte word
        assert self.n % self.per == 0
        self.words = self.n // self.per
        self.t = torch.full((self.words + 2 * GUARD,), SENT, dtype=torch.int32, device=dev)
        if init is not None:
            self.t[GUARD:GUARD + self.words] = torch.from_numpy(np.ascontiguousarray(init, self.dtype).ravel().view(np.int32)).to(dev)

    def ptr(self):
        return self.t.data_ptr() + 4 * GUARD

    def body_words(self):
        torch.cuda.synchronize()
        return self.t[GUARD:GUARD + self.words]

    def dev(self, torch_dtype):
        """The body as a device tensor of ``torch_dtype`` (same element size as ``dtype``)."""
        return self.body_words().view(torch_dtype)

    def read(self):
        return self.body_words().cpu().numpy().view(self.dtype).copy()

    def guards_intact(self):
        torch.cuda.synchronize()
        g = torch.cat([self.t[:GUARD], self.t[GUARD + self.words:]])
        return bool((g == SENT).all())

    def untouched(self, first_word=0):
        """Number of body words from ``first_word`` on that still hold the sentinel."""
        return int((self.body_words()[first_word:] == SENT).sum())


def dv(dev, a, dtype=f32):
    a = np.ascontiguousarray(a, dtype)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(dev)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)


def bits16(a):
    return np.ascontiguousarray(a, f16).view(np.uint16)


def ratio(got, ref, bound):
    """Worst |got - ref| / bound (0 where the difference is 0, so a zero bound demands equality; NaN if got has one)."""
    err = np.abs(np.asarray(got, f64) - np.asarray(ref, f64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / np.maximum(np.asarray(bound, f64), 1e-300))
    return float(np.max(r)) if r.size else 0.0


def relmax(got, ref):
    return float(np.abs(np.asarray(got, f64) - ref).max() / max(float(np.abs(ref).max()), 1e-300))


def _args(args):
    h = _hip()
    return [a.ptr() if isinstance(a, Out) else h.ptr(a) if isinstance(a, torch.Tensor) else a for a in args]


def call(name, *args):
    h = _hip()
    h.call(name, *_args(args), h.stream())


def status(name, *args):
    h = _hip()
    return getattr(h.load(), name)(*_args(args), h.stream())


def pair_ok(hi, lo, v64, extra=0.0):
    """Worst ratio of |hi + lo - v| to 2^-22 |v| + 2^-25 + extra."""
    v64 = np.asarray(v64, f64)
    return ratio(hi.astype(f64) + lo.astype(f64), v64, 2.0 ** -22 * np.abs(v64) + 2.0 ** -25 + extra)


def normal16(v):
    a = np.abs(v)
    return (a >= 2.0 ** -14) & (a <= 65504.0)

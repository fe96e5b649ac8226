"""K21: one short least-squares FIR per clip that carries a rendered wet onto a recorded one, forward and backward on the
device (csrc/fir_match.hip; include/modex_hip.h has the definition) -- no counterpart in the reference.

    x = y_hat, both rows zero outside [0, N);  K taps, a centre c
    R[d] = sum_n x[n] x[n + d],  b[j] = sum_n x[n + c - j] y[n],  E = sum_n y[n]^2      (fp64 sums of exact products)
    A = toeplitz(R) + (eps + ridge R[0]) I,  h = A^-1 b (fp64 Cholesky), rounded once to fp32
    z[n] = sum_k h[k] x[n + c - k]                                                     (fp64, rounded once)
    flags: 1 = a pivot that is not positive or not finite, 2 = not (sum |h| <= max_gain); a flagged row gets the
    identity filter (h[c] = 1) and passes its gradient through unchanged

    backward:  gh[k] = sum_n dz[n] x[n + c - k],  u = A^-1 gh,  s = the 2K - 1 lags of h (x) u + u (x) h, s[0] += 2 ridge <u, h>
               dy_hat[i] = sum_k h[k] dz[i + k - c] + sum_k u[k] y[i + k - c] - sum_d s[d] x[i + d]

K = 1 is ``gain.match_gain``'s "ls" gain; a centred window also absorbs a lag of a fraction of a sample, and K taps a tone
curve of that length.  ``lightning.LFOExtractionThroughEffect(match_fir=...)`` is the user.  Everything here returns device
tensors and never synchronises with the host.  ``y`` gets no gradient.
"""
import math
from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor as T
from torch import nn

from . import _hip
from .gain import _out_rows, _overlap, _pair, _rows, _stride

CHUNK = 2048                                    # samples a workgroup owns (MX_FIR_CHUNK)
MAX_TAPS = 32                                   # MX_FIR_MAX_TAPS


class FirMatch(NamedTuple):
    """What ``match_fir`` returns: ``z`` the matched rows, of ``y_hat``'s shape; ``taps`` (B, K) fp32, the applied h; ``sums``
    (B, 2K + 1) fp64 = R, b, E; ``flags`` (B,) int32 (0, or 1 / 2: which guard gave the row the identity filter)."""
    z: T
    taps: T
    sums: T
    flags: T


def _number(v, lo: float, strict: bool) -> bool:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not v < math.inf:
        return False
    return v > lo if strict else v >= lo


def check_fir(taps, centre, ridge, eps, max_gain, fn: str) -> Tuple[int, int, float, float, float]:
    """(K, centre, ridge, eps, max_gain) or the ValueError that names the bad argument; ``centre=None`` is (K - 1) // 2."""
    if isinstance(taps, bool) or not isinstance(taps, int) or not 1 <= taps <= MAX_TAPS:
        raise ValueError(f"{fn}: taps must be an integer in 1 .. {MAX_TAPS}, got {taps!r}")
    if centre is None:
        centre = (taps - 1) // 2
    if isinstance(centre, bool) or not isinstance(centre, int) or not 0 <= centre < taps:
        raise ValueError(f"{fn}: centre must be an integer in 0 .. taps - 1 = {taps - 1} (or None), got {centre!r}")
    if not _number(ridge, 0.0, False):
        raise ValueError(f"{fn}: ridge must be a finite number >= 0, got {ridge!r}")
    if not _number(eps, 0.0, True):
        raise ValueError(f"{fn}: eps must be a finite number above 0, got {eps!r}")
    if not _number(max_gain, 1.0, False):
        raise ValueError(f"{fn}: max_gain must be a finite number >= 1, got {max_gain!r}")
    return taps, centre, float(ridge), float(eps), float(max_gain)


def n_chunks(N: int) -> int:
    return (N + CHUNK - 1) // CHUNK


def match_fir(y_hat: T, y: T, taps: int = 9, centre: Optional[int] = None, ridge: float = 1e-6, eps: float = 1e-8,
              max_gain: float = 20.0, out: Optional[T] = None) -> FirMatch:
    """``FirMatch(z, taps, sums, flags)`` for fp32 device tensors ``y_hat`` and ``y`` of one shape, (B, N) or (B, 1, N), in
    three launches (``mx_fir_match_partials``, ``mx_fir_match_solve``, ``mx_fir_match_apply``).  Rows a row stride apart
    (inner stride 1) are read in place, wherever they start.  ``out`` (fp32, ``y_hat``'s shape, inner stride 1) receives
    ``z``; it may overlap neither input."""
    fn = "match_fir"
    K, c, ridge, eps, max_gain = check_fir(taps, centre, ridge, eps, max_gain, fn)
    p, q = _pair(y_hat, y, fn)
    B, N = p.shape
    if out is None:
        out = torch.empty(y_hat.shape, device=p.device, dtype=torch.float32)
    o = _out_rows(out, y_hat, "out", fn)
    if _overlap(o, p) or _overlap(o, q):
        raise ValueError(f"{fn}: out may not overlap y_hat or y")
    nc = n_chunks(N)
    partials = torch.empty((B, nc, 2 * K + 1), device=p.device, dtype=torch.float64)
    h = torch.empty((B, K), device=p.device, dtype=torch.float32)
    sums = torch.empty((B, 2 * K + 1), device=p.device, dtype=torch.float64)
    flags = torch.empty(B, device=p.device, dtype=torch.int32)
    _hip.call("mx_fir_match_partials", p.data_ptr(), _stride(p), q.data_ptr(), _stride(q), B, N, K, c, _hip.ptr(partials),
              _hip.stream())
    _hip.call("mx_fir_match_solve", _hip.ptr(partials), B, nc, K, c, ridge, eps, max_gain, _hip.ptr(h), _hip.ptr(sums),
              _hip.ptr(flags), _hip.stream())
    _hip.call("mx_fir_match_apply", p.data_ptr(), _stride(p), _hip.ptr(h), B, N, K, c, o.data_ptr(), _stride(o), _hip.stream())
    return FirMatch(out, h, sums, flags)


def match_fir_backward(dz: T, y_hat: T, y: T, match: FirMatch, ridge: float, eps: float, centre: int,
                       out: Optional[T] = None) -> T:
    """d loss / d y_hat from ``dz`` = d loss / d z, of ``y_hat``'s shape, in three launches (``mx_fir_match_bwd_partials``,
    ``mx_fir_match_bwd_solve``, ``mx_fir_match_bwd_apply``).  ``y_hat`` and ``y`` are the forward's inputs, ``match`` what it
    returned (its taps, sums and flags are read; K is the taps' width).  ``ridge``, ``eps`` and ``centre`` are the forward's and
    have no defaults here: a ``FirMatch`` does not carry them, and a backward with another centre than the forward's would be a
    wrong gradient without a sign of it (``centre`` is the integer the forward used, (K - 1) // 2 for its ``centre=None``).
    ``out`` may overlap none of ``dz``, ``y_hat``, ``y``: a sample's gradient reads its neighbours' ``dz``, so there is no
    in-place update."""
    return _backward_parts(dz, y_hat, y, match, ridge, eps, centre, out)[0]


def _backward_parts(dz, y_hat, y, match, ridge, eps, centre, out=None) -> Tuple[T, T, T, T]:
    """``match_fir_backward`` with its intermediates: (dy_hat, partials (B, n_chunks, K), u (B, K), s (B, 2K - 1)), the last
    three fp64 device tensors (the kernel-level tests check each stage)."""
    fn = "match_fir_backward"
    if not isinstance(match, FirMatch):
        raise ValueError(f"{fn}: match must be the FirMatch of the forward")
    if not isinstance(match.taps, torch.Tensor) or match.taps.ndim != 2:
        raise ValueError(f"{fn}: match.taps must be a torch.float32 tensor of shape (B, K) on y_hat's device")
    if centre is None:
        raise ValueError(f"{fn}: centre must be the integer the forward used ((K - 1) // 2 for its centre=None), got None")
    K, c, ridge, eps, _ = check_fir(match.taps.size(1), centre, ridge, eps, 1.0, fn)
    p, q = _pair(y_hat, y, fn)
    B, N = p.shape
    d = _rows(dz, "dz", fn)
    if d.shape != p.shape or d.device != p.device:
        raise ValueError(f"{fn}: dz must have y_hat's rows on its device, got {tuple(d.shape)}")
    for name, t, shape, dtype in (("taps", match.taps, (B, K), torch.float32), ("sums", match.sums, (B, 2 * K + 1), torch.float64),
                                  ("flags", match.flags, (B,), torch.int32)):
        if not isinstance(t, torch.Tensor) or t.shape != shape or t.dtype != dtype or t.device != p.device:
            raise ValueError(f"{fn}: match.{name} must be a {dtype} tensor of shape {shape} on y_hat's device")
    if out is None:
        out = torch.empty(y_hat.shape, device=p.device, dtype=torch.float32)
    o = _out_rows(out, y_hat, "out", fn)
    if _overlap(o, d) or _overlap(o, p) or _overlap(o, q):
        raise ValueError(f"{fn}: out may not overlap dz, y_hat or y (there is no in-place update)")
    nc = n_chunks(N)
    partials = torch.empty((B, nc, K), device=p.device, dtype=torch.float64)
    u = torch.empty((B, K), device=p.device, dtype=torch.float64)
    s = torch.empty((B, 2 * K - 1), device=p.device, dtype=torch.float64)
    h, sums, flags = match.taps.contiguous(), match.sums.contiguous(), match.flags.contiguous()
    _hip.call("mx_fir_match_bwd_partials", d.data_ptr(), _stride(d), p.data_ptr(), _stride(p), B, N, K, c, _hip.ptr(partials),
              _hip.stream())
    _hip.call("mx_fir_match_bwd_solve", _hip.ptr(partials), _hip.ptr(sums), _hip.ptr(h), _hip.ptr(flags), B, nc, K, ridge, eps,
              _hip.ptr(u), _hip.ptr(s), _hip.stream())
    _hip.call("mx_fir_match_bwd_apply", d.data_ptr(), _stride(d), q.data_ptr(), _stride(q), p.data_ptr(), _stride(p), _hip.ptr(h),
              _hip.ptr(u), _hip.ptr(s), B, N, K, c, o.data_ptr(), _stride(o), _hip.stream())
    return out, partials, u, s


class _MatchFirFn(torch.autograd.Function):
    """z = match_fir(y_hat, y) as one autograd node: the forward's three launches, the backward's three."""

    @staticmethod
    def forward(ctx, y_hat, y, taps, centre, ridge, eps, max_gain):
        m = match_fir(y_hat, y, taps, centre, ridge, eps, max_gain)
        ctx.save_for_backward(y_hat, y, m.taps, m.sums, m.flags)
        ctx.centre, ctx.ridge, ctx.eps = (m.taps.size(1) - 1) // 2 if centre is None else centre, ridge, eps
        ctx.mark_non_differentiable(m.taps, m.sums, m.flags)
        return m.z, m.taps, m.sums, m.flags

    @staticmethod
    def backward(ctx, dz, *_):
        y_hat, y, taps, sums, flags = ctx.saved_tensors
        d = match_fir_backward(dz.contiguous(), y_hat, y, FirMatch(dz, taps, sums, flags), ctx.ridge, ctx.eps, ctx.centre)
        return d, None, None, None, None, None, None


class MatchFir(nn.Module):
    """``forward(y_hat, y)`` = ``match_fir(y_hat, y, taps, centre, ridge, eps, max_gain).z``, differentiable in ``y_hat``
    through one autograd node; ``y`` gets no gradient.  ``last`` holds the ``FirMatch`` of the latest call (device tensors)."""

    def __init__(self, taps: int = 9, centre: Optional[int] = None, ridge: float = 1e-6, eps: float = 1e-8,
                 max_gain: float = 20.0) -> None:
        super().__init__()
        self.taps, self.centre, self.ridge, self.eps, self.max_gain = check_fir(taps, centre, ridge, eps, max_gain, "MatchFir")
        self.last: Optional[FirMatch] = None

    def forward(self, y_hat: T, y: T) -> T:
        self.last = FirMatch(*_MatchFirFn.apply(y_hat, y, self.taps, self.centre, self.ridge, self.eps, self.max_gain))
        return self.last.z

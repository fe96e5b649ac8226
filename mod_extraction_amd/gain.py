"""K20: one gain per clip that carries a rendered wet onto a recorded one, forward and backward on the device
(csrc/gain_match.hip; include/modex_hip.h, K20, has the definition) -- no counterpart in the reference.

    a = <y_hat, y_hat>,  c = <y_hat, y>,  e = <y, y>          (fp64 sums of exact products, a fixed order)
    "ls":  g = c / (a + eps)             "rms":  g = sqrt((e + eps) / (a + eps))
    gain_range = (lo, hi): g is clamped into it and the row flagged;  g is rounded once to fp32;  z = fl32(g * y_hat)

    backward, s = <dz, y_hat>:   "ls"   dy_hat = g dz + s (y - 2 g y_hat) / (a + eps)
                                 "rms"  dy_hat = g dz - s g y_hat / (a + eps)          a clamped row: dy_hat = g dz

A recorded wet is never at the level of the project's own render of the dry, and no effect here has a gain of its own:
``lightning.LFOExtractionThroughEffect(match_gain=...)`` is the user.  Everything here returns device tensors and never
synchronises with the host.  ``y`` gets no gradient.
"""
import math
from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor as T
from torch import nn

from . import _hip

CHUNK = 2048                                    # samples a workgroup owns (MX_GAIN_CHUNK)
MODES = ("ls", "rms")                           # their index is the kernels' mode code


class GainMatch(NamedTuple):
    """What ``match_gain`` returns: ``z`` the matched rows, of ``y_hat``'s shape; ``gain`` (B,) fp32, the applied g; ``sums``
    (B, 3) fp64 = a, c, e; ``flags`` (B,) int32, 1 where the gain was clamped."""
    z: T
    gain: T
    sums: T
    flags: T


def _rows(x, name: str, fn: str) -> T:
    """(B, N) view of an fp32 device tensor of shape (B, N) or (B, 1, N); rows a row stride apart are left in place."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.ndim not in (2, 3) or (x.ndim == 3 and x.size(1) != 1):
        raise ValueError(f"{fn}: {name} must be an fp32 tensor of shape (B, N) or (B, 1, N)")
    if not x.is_cuda:
        raise ValueError(f"{fn}: {name} must be on a HIP device (there is no CPU fallback)")
    x = x.detach()
    x = x[:, 0, :] if x.ndim == 3 else x
    B, N = x.shape
    if B == 0 or N == 0:
        raise ValueError(f"{fn}: {name} has no rows or no samples")
    if x.stride(1) != 1 or (B > 1 and x.stride(0) < N):
        x = x.contiguous()
    return x


def _stride(x: T) -> int:
    return max(x.stride(0), x.size(1)) if x.size(0) > 1 else x.size(1)


def _out_rows(out, like: T, name: str, fn: str) -> T:
    """The (B, N) view of a caller's ``out`` (of ``like``'s shape), which is written in place and so is never copied."""
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.shape != like.shape or out.device != like.device:
        raise ValueError(f"{fn}: {name} must be an fp32 tensor of shape {tuple(like.shape)} on the inputs' device")
    o = out[:, 0, :] if out.ndim == 3 else out
    if o.stride(1) != 1 or (o.size(0) > 1 and o.stride(0) < o.size(1)):
        raise ValueError(f"{fn}: {name} needs inner stride 1 and rows at least N = {o.size(1)} floats apart")
    return o


def _overlap(a: T, b: T) -> bool:
    B, N = a.shape
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + 4 * ((B - 1) * _stride(b) + N) and b0 < a0 + 4 * ((B - 1) * _stride(a) + N)


def check_mode(mode, eps, gain_range, fn: str) -> Tuple[int, float, Optional[Tuple[float, float]]]:
    """(mode code, eps, range) or the ValueError that says which of the three is wrong."""
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"{fn}: mode must be one of {MODES}, got {mode!r}")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not (0.0 < eps < math.inf):
        raise ValueError(f"{fn}: eps must be a finite number above 0, got {eps!r}")
    if gain_range is not None:
        ok = isinstance(gain_range, (tuple, list)) and len(gain_range) == 2 and all(
            isinstance(v, (int, float)) and not isinstance(v, bool) for v in gain_range)
        if not ok or not (0.0 < gain_range[0] <= 1.0 <= gain_range[1] < math.inf):
            raise ValueError(f"{fn}: gain_range must be (lo, hi) with 0 < lo <= 1 <= hi, got {gain_range!r}")
        gain_range = (float(gain_range[0]), float(gain_range[1]))
    return MODES.index(mode), float(eps), gain_range


def _pair(y_hat, y, fn: str) -> Tuple[T, T]:
    p, q = _rows(y_hat, "y_hat", fn), _rows(y, "y", fn)
    if p.shape != q.shape or p.device != q.device:
        raise ValueError(f"{fn}: y_hat and y must have the same rows on the same device, got {tuple(p.shape)} and {tuple(q.shape)}")
    return p, q


def n_chunks(N: int) -> int:
    return (N + CHUNK - 1) // CHUNK


def match_gain(y_hat: T, y: T, mode: str = "ls", eps: float = 1e-8, gain_range: Optional[Tuple[float, float]] = None,
               out: Optional[T] = None) -> GainMatch:
    """``GainMatch(z, gain, sums, flags)`` for fp32 device tensors ``y_hat`` and ``y`` of one shape, (B, N) or (B, 1, N), in two
    launches (``mx_gain_match_partials``, ``mx_gain_match_apply``).  Rows a row stride apart (inner stride 1) are read in
    place, wherever they start.  ``out`` (fp32, ``y_hat``'s shape, inner stride 1) receives ``z``; it may overlap neither
    input."""
    fn = "match_gain"
    code, eps, rng = check_mode(mode, eps, gain_range, fn)
    p, q = _pair(y_hat, y, fn)
    B, N = p.shape
    if out is None:
        out = torch.empty(y_hat.shape, device=p.device, dtype=torch.float32)
    o = _out_rows(out, y_hat, "out", fn)
    if _overlap(o, p) or _overlap(o, q):
        raise ValueError(f"{fn}: out may not overlap y_hat or y")
    partials = torch.empty((B, n_chunks(N), 3), device=p.device, dtype=torch.float64)
    gain = torch.empty(B, device=p.device, dtype=torch.float32)
    sums = torch.empty((B, 3), device=p.device, dtype=torch.float64)
    flags = torch.empty(B, device=p.device, dtype=torch.int32)
    _hip.call("mx_gain_match_partials", p.data_ptr(), _stride(p), q.data_ptr(), _stride(q), B, N, _hip.ptr(partials),
              _hip.stream())
    lo, hi = rng if rng is not None else (0.0, 0.0)
    _hip.call("mx_gain_match_apply", p.data_ptr(), _stride(p), _hip.ptr(partials), B, N, code, eps, int(rng is not None), lo, hi,
              o.data_ptr(), _stride(o), _hip.ptr(gain), _hip.ptr(sums), _hip.ptr(flags), _hip.stream())
    return GainMatch(out, gain, sums, flags)


def match_gain_backward(dz: T, y_hat: T, y: T, match: GainMatch, mode: str = "ls", eps: float = 1e-8,
                        out: Optional[T] = None) -> T:
    """d loss / d y_hat from ``dz`` = d loss / d z, of ``y_hat``'s shape, in two launches (``mx_gain_match_bwd_partials``,
    ``mx_gain_match_bwd_apply``).  ``y_hat`` and ``y`` are the forward's inputs, ``match`` what it returned (its gain, sums and
    flags are read; the clamp is in the flags), ``mode`` and ``eps`` the forward's.  ``out=dz`` updates ``dz`` in place; any other
    ``out`` may overlap none of the three."""
    fn = "match_gain_backward"
    code, eps, _ = check_mode(mode, eps, None, fn)
    p, q = _pair(y_hat, y, fn)
    B, N = p.shape
    in_place = out is dz
    d = _out_rows(dz, y_hat, "dz", fn) if in_place else _rows(dz, "dz", fn)
    if d.shape != p.shape or d.device != p.device:
        raise ValueError(f"{fn}: dz must have y_hat's rows on its device, got {tuple(d.shape)}")
    if not isinstance(match, GainMatch):
        raise ValueError(f"{fn}: match must be the GainMatch of the forward")
    for name, t, shape, dtype in (("gain", match.gain, (B,), torch.float32), ("sums", match.sums, (B, 3), torch.float64),
                                  ("flags", match.flags, (B,), torch.int32)):
        if not isinstance(t, torch.Tensor) or t.shape != shape or t.dtype != dtype or t.device != p.device:
            raise ValueError(f"{fn}: match.{name} must be a {dtype} tensor of shape {shape} on y_hat's device")
    if out is None:
        out = torch.empty(y_hat.shape, device=p.device, dtype=torch.float32)
    o = d if in_place else _out_rows(out, y_hat, "out", fn)
    if (not in_place and _overlap(o, d)) or _overlap(o, p) or _overlap(o, q):
        raise ValueError(f"{fn}: out may be dz itself; it may not overlap dz otherwise, nor y_hat or y")
    partials = torch.empty((B, n_chunks(N)), device=p.device, dtype=torch.float64)
    _hip.call("mx_gain_match_bwd_partials", d.data_ptr(), _stride(d), p.data_ptr(), _stride(p), B, N, _hip.ptr(partials),
              _hip.stream())
    _hip.call("mx_gain_match_bwd_apply", d.data_ptr(), _stride(d), p.data_ptr(), _stride(p), q.data_ptr(), _stride(q),
              _hip.ptr(match.gain.contiguous()), _hip.ptr(match.sums.contiguous()), _hip.ptr(match.flags.contiguous()),
              _hip.ptr(partials), B, N, code, eps, o.data_ptr(), _stride(o), _hip.stream())
    return out


class _MatchGainFn(torch.autograd.Function):
    """z = match_gain(y_hat, y) as one autograd node: the forward's two launches, the backward's two."""

    @staticmethod
    def forward(ctx, y_hat, y, mode, eps, gain_range):
        m = match_gain(y_hat, y, mode, eps, gain_range)
        ctx.save_for_backward(y_hat, y, m.gain, m.sums, m.flags)
        ctx.mode, ctx.eps = mode, eps
        ctx.mark_non_differentiable(m.gain, m.sums, m.flags)
        return m.z, m.gain, m.sums, m.flags

    @staticmethod
    def backward(ctx, dz, *_):
        y_hat, y, gain, sums, flags = ctx.saved_tensors
        d = match_gain_backward(dz.contiguous(), y_hat, y, GainMatch(dz, gain, sums, flags), ctx.mode, ctx.eps)
        return d, None, None, None, None


class MatchGain(nn.Module):
    """``forward(y_hat, y)`` = ``match_gain(y_hat, y, mode, eps, gain_range).z``, differentiable in ``y_hat`` through one
    autograd node; ``y`` gets no gradient.  ``last`` holds the ``GainMatch`` of the latest call (device tensors)."""

    def __init__(self, mode: str = "ls", eps: float = 1e-8, gain_range: Optional[Tuple[float, float]] = None) -> None:
        super().__init__()
        check_mode(mode, eps, gain_range, "MatchGain")
        self.mode, self.eps, self.gain_range = mode, eps, gain_range
        self.last: Optional[GainMatch] = None

    def forward(self, y_hat: T, y: T) -> T:
        self.last = GainMatch(*_MatchGainFn.apply(y_hat, y, self.mode, self.eps, self.gain_range))
        return self.last.z

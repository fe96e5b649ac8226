"""K27: one memoryless polynomial curve per clip that carries a rendered wet onto a recorded one that went through a
saturating stage, forward and backward on the device (csrc/shaper_match.hip; csrc/shaper_match_abi.h has the definition) -- no
counterpart in the reference.

    x = y_hat;  order P in 1 .. 7;  powers p_1 < .. < p_K: the odd integers <= P, with ``even`` all of 1 .. P;  no constant term
    S2 = sum x^2,  r = fl32(sqrt(S2 / N)),  t = x / r                                    (fp64 sums in a fixed order)
    A[i][j] = sum t^(p_i + p_j), the diagonal times (1 + ridge);  b_k = sum t^(p_k) y / r;  c = A^-1 b (fp64 Cholesky), fp32
    z = fl32(r sum_k c_k t^(p_k))
    flags: 1 = S2, r or a pivot not positive or not finite, 2 = not (sum |c| <= max_gain); a flagged row gets the identity
    (c_1 = 1, z = y_hat bit for bit) and passes its gradient through unchanged

    backward:  g_k = sum dz t^(p_k),  u = A^-1 g,  C(t) = sum c_k t^(p_k),  U(t) = sum u_k t^(p_k)
               dy_hat = dz C'(t) + U'(t) y / r - (U'(t) C(t) + U(t) C'(t)) - 2 ridge sum_k u_k c_k p_k t^(2 p_k - 1)

Order 1 is ``gain.match_gain``'s "ls" gain; an odd quintic takes a soft clip (a compander, an op-amp stage, a re-amp box) down
by two orders of magnitude, and asymmetric curves need ``even``.  There is no absolute eps: the fit is exactly independent of
the level of ``y_hat``.  ``lightning.LFOExtractionThroughEffect(match_shaper=...)`` is the user.  Everything here returns device
tensors and never synchronises with the host.  ``y`` gets no gradient.
"""
from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor as T
from torch import nn

from . import _hip
from .fir_match import _number
from .gain import _out_rows, _overlap, _pair, _rows, _stride

CHUNK = _hip.SHAPER_CHUNK                       # samples a workgroup owns (MX_SHAPER_CHUNK)
MAX_ORDER = _hip.SHAPER_MAX_ORDER               # MX_SHAPER_MAX_ORDER


class ShaperMatch(NamedTuple):
    """What ``match_shaper`` returns: ``z`` the shaped rows, of ``y_hat``'s shape; ``coeffs`` (B, K) fp32, the applied c;
    ``scale`` (B,) fp32, r; ``sums`` (B, n_sums) fp64 = S2, the moments in ascending order, b, E; ``flags`` (B,) int32 (0, or
    1 / 2: which guard gave the row the identity)."""
    z: T
    coeffs: T
    scale: T
    sums: T
    flags: T


def powers(order: int, even: bool = False) -> Tuple[int, ...]:
    """p_1 < .. < p_K: the odd integers <= ``order``, with ``even`` every integer in 1 .. ``order``."""
    return tuple(p for p in range(1, order + 1) if even or p % 2)


def n_sums(order: int, even: bool = False) -> int:
    """S2, the moments m = p_i + p_j, the K cross sums, E."""
    p = powers(order, even)
    return 1 + len({a + b for a in p for b in p}) + len(p) + 1


def check_shaper(order, even, ridge, max_gain, fn: str) -> Tuple[int, bool, float, float]:
    """(order, even, ridge, max_gain) or the ValueError that names the bad argument."""
    if isinstance(order, bool) or not isinstance(order, int) or not 1 <= order <= MAX_ORDER:
        raise ValueError(f"{fn}: order must be an integer in 1 .. {MAX_ORDER}, got {order!r}")
    if not isinstance(even, bool):
        raise ValueError(f"{fn}: even must be True or False, got {even!r}")
    if not _number(ridge, 0.0, False):
        raise ValueError(f"{fn}: ridge must be a finite number >= 0, got {ridge!r}")
    if not _number(max_gain, 1.0, False):
        raise ValueError(f"{fn}: max_gain must be a finite number >= 1, got {max_gain!r}")
    return order, even, float(ridge), float(max_gain)


def n_chunks(N: int) -> int:
    return (N + CHUNK - 1) // CHUNK


def match_shaper(y_hat: T, y: T, order: int = 5, even: bool = False, ridge: float = 1e-9, max_gain: float = 20.0,
                 out: Optional[T] = None) -> ShaperMatch:
    """``ShaperMatch(z, coeffs, scale, sums, flags)`` for fp32 device tensors ``y_hat`` and ``y`` of one shape, (B, N) or
    (B, 1, N), in three calls (``mx_shaper_match_partials``, ``mx_shaper_match_solve``, ``mx_shaper_match_apply``).  Rows a row
    stride apart (inner stride 1) are read in place, wherever they start.  ``out`` (fp32, ``y_hat``'s shape, inner stride 1)
    receives ``z``; it may overlap neither input."""
    return _forward_parts(y_hat, y, order, even, ridge, max_gain, out)[0]


def _forward_parts(y_hat, y, order, even, ridge, max_gain, out=None) -> Tuple[ShaperMatch, T]:
    """``match_shaper`` with its workspace: (ShaperMatch, partials (B, n_chunks, n_sums) fp64) -- the kernel-level tests check
    each stage."""
    fn = "match_shaper"
    order, even, ridge, max_gain = check_shaper(order, even, ridge, max_gain, fn)
    p, q = _pair(y_hat, y, fn)
    B, N = p.shape
    if out is None:
        out = torch.empty(y_hat.shape, device=p.device, dtype=torch.float32)
    o = _out_rows(out, y_hat, "out", fn)
    if _overlap(o, p) or _overlap(o, q):
        raise ValueError(f"{fn}: out may not overlap y_hat or y")
    nc, ns, K = n_chunks(N), n_sums(order, even), len(powers(order, even))
    partials = torch.empty((B, nc, ns), device=p.device, dtype=torch.float64)
    coeffs = torch.empty((B, K), device=p.device, dtype=torch.float32)
    scale = torch.empty(B, device=p.device, dtype=torch.float32)
    sums = torch.empty((B, ns), device=p.device, dtype=torch.float64)
    flags = torch.empty(B, device=p.device, dtype=torch.int32)
    _hip.call("mx_shaper_match_partials", p.data_ptr(), _stride(p), q.data_ptr(), _stride(q), B, N, order, int(even),
              _hip.ptr(partials), _hip.stream())
    _hip.call("mx_shaper_match_solve", _hip.ptr(partials), B, N, nc, order, int(even), ridge, max_gain, _hip.ptr(coeffs),
              _hip.ptr(scale), _hip.ptr(sums), _hip.ptr(flags), _hip.stream())
    _hip.call("mx_shaper_match_apply", p.data_ptr(), _stride(p), _hip.ptr(coeffs), _hip.ptr(scale), _hip.ptr(flags), B, N, order,
              int(even), o.data_ptr(), _stride(o), _hip.stream())
    return ShaperMatch(out, coeffs, scale, sums, flags), partials


def match_shaper_backward(dz: T, y_hat: T, y: T, match: ShaperMatch, even: bool, ridge: float, out: Optional[T] = None) -> T:
    """d loss / d y_hat from ``dz`` = d loss / d z, of ``y_hat``'s shape, in three calls (``mx_shaper_match_bwd_partials``,
    ``mx_shaper_match_bwd_solve``, ``mx_shaper_match_bwd_apply``).  ``y_hat`` and ``y`` are the forward's inputs, ``match`` what
    it returned (its coeffs, scale, sums and flags are read).  ``even`` and ``ridge`` are the forward's and have no defaults
    here: a ``ShaperMatch`` does not carry them, and the width of ``coeffs`` with ``even`` gives the order back (an even order
    without ``even`` is the odd order below it).  ``out=dz`` updates ``dz`` in place; any other ``out`` may overlap none of
    the three."""
    return _backward_parts(dz, y_hat, y, match, even, ridge, out)[0]


def _backward_parts(dz, y_hat, y, match, even, ridge, out=None) -> Tuple[T, T, T]:
    """``match_shaper_backward`` with its intermediates: (dy_hat, partials (B, n_chunks, K), u (B, K)), the last two fp64."""
    fn = "match_shaper_backward"
    if not isinstance(match, ShaperMatch):
        raise ValueError(f"{fn}: match must be the ShaperMatch of the forward")
    if not isinstance(match.coeffs, torch.Tensor) or match.coeffs.ndim != 2 or not 1 <= match.coeffs.size(1) <= MAX_ORDER:
        raise ValueError(f"{fn}: match.coeffs must be a torch.float32 tensor of shape (B, K) on y_hat's device")
    if not isinstance(even, bool):
        raise ValueError(f"{fn}: even must be the forward's True or False, got {even!r}")
    K = match.coeffs.size(1)
    order = K if even else 2 * K - 1
    order, even, ridge, _ = check_shaper(order, even, ridge, 1.0, fn)
    p, q = _pair(y_hat, y, fn)
    B, N = p.shape
    in_place = out is dz
    d = _out_rows(dz, y_hat, "dz", fn) if in_place else _rows(dz, "dz", fn)
    if d.shape != p.shape or d.device != p.device:
        raise ValueError(f"{fn}: dz must have y_hat's rows on its device, got {tuple(d.shape)}")
    ns = n_sums(order, even)
    for name, t, shape, dtype in (("coeffs", match.coeffs, (B, K), torch.float32), ("scale", match.scale, (B,), torch.float32),
                                  ("sums", match.sums, (B, ns), torch.float64), ("flags", match.flags, (B,), torch.int32)):
        if not isinstance(t, torch.Tensor) or t.shape != shape or t.dtype != dtype or t.device != p.device:
            raise ValueError(f"{fn}: match.{name} must be a {dtype} tensor of shape {shape} on y_hat's device")
    if out is None:
        out = torch.empty(y_hat.shape, device=p.device, dtype=torch.float32)
    o = d if in_place else _out_rows(out, y_hat, "out", fn)
    if (not in_place and _overlap(o, d)) or _overlap(o, p) or _overlap(o, q):
        raise ValueError(f"{fn}: out may be dz itself; it may not overlap dz otherwise, nor y_hat or y")
    nc = n_chunks(N)
    partials = torch.empty((B, nc, K), device=p.device, dtype=torch.float64)
    u = torch.empty((B, K), device=p.device, dtype=torch.float64)
    c, r, sums, flags = (match.coeffs.contiguous(), match.scale.contiguous(), match.sums.contiguous(), match.flags.contiguous())
    _hip.call("mx_shaper_match_bwd_partials", d.data_ptr(), _stride(d), p.data_ptr(), _stride(p), _hip.ptr(r), B, N, order,
              int(even), _hip.ptr(partials), _hip.stream())
    _hip.call("mx_shaper_match_bwd_solve", _hip.ptr(partials), _hip.ptr(sums), _hip.ptr(flags), B, nc, order, int(even), ridge,
              _hip.ptr(u), _hip.stream())
    _hip.call("mx_shaper_match_bwd_apply", d.data_ptr(), _stride(d), p.data_ptr(), _stride(p), q.data_ptr(), _stride(q),
              _hip.ptr(c), _hip.ptr(r), _hip.ptr(u), _hip.ptr(flags), B, N, order, int(even), ridge, o.data_ptr(), _stride(o),
              _hip.stream())
    return out, partials, u


class _MatchShaperFn(torch.autograd.Function):
    """z = match_shaper(y_hat, y) as one autograd node: the forward's three calls, the backward's three."""

    @staticmethod
    def forward(ctx, y_hat, y, order, even, ridge, max_gain):
        m = match_shaper(y_hat, y, order, even, ridge, max_gain)
        ctx.save_for_backward(y_hat, y, m.coeffs, m.scale, m.sums, m.flags)
        ctx.even, ctx.ridge = even, ridge
        ctx.mark_non_differentiable(m.coeffs, m.scale, m.sums, m.flags)
        return m.z, m.coeffs, m.scale, m.sums, m.flags

    @staticmethod
    def backward(ctx, dz, *_):
        y_hat, y, coeffs, scale, sums, flags = ctx.saved_tensors
        d = match_shaper_backward(dz.contiguous(), y_hat, y, ShaperMatch(dz, coeffs, scale, sums, flags), ctx.even, ctx.ridge)
        return d, None, None, None, None, None


class MatchShaper(nn.Module):
    """``forward(y_hat, y)`` = ``match_shaper(y_hat, y, order, even, ridge, max_gain).z``, differentiable in ``y_hat`` through
    one autograd node; ``y`` gets no gradient.  ``last`` holds the ``ShaperMatch`` of the latest call (device tensors)."""

    def __init__(self, order: int = 5, even: bool = False, ridge: float = 1e-9, max_gain: float = 20.0) -> None:
        super().__init__()
        self.order, self.even, self.ridge, self.max_gain = check_shaper(order, even, ridge, max_gain, "MatchShaper")
        self.last: Optional[ShaperMatch] = None

    def forward(self, y_hat: T, y: T) -> T:
        self.last = ShaperMatch(*_MatchShaperFn.apply(y_hat, y, self.order, self.even, self.ridge, self.max_gain))
        return self.last.z

"""K19: the constant lag and the polarity of recorded dry / wet pairs, by cross-correlation on the device
(csrc/pair_align.hip; include/modex_hip.h, K19, has the definition) -- no counterpart in the reference.

    r[b, l + L] = sum_n dry[b, n] wet[b, n + l],  l = -L..L;   c = r / sqrt(sum dry^2 sum wet^2)
    lag = argmax |c| (ties: smallest |l|, then l >= 0);  corr = c[lag];  frac = the parabolic sub-sample offset

Convention: ``wet[n + lag] ~ sign(corr) * dry[n]``: a wet that is late by d samples has ``lag = +d``, and
``shift_rows(wet, lag, corr)`` lines it up with ``dry``.  Everything here returns device tensors and never synchronises with
the host.  ``datasets.RandomAudioChunkDryWetDataset.estimate_alignment`` is the user of the estimate: one integer lag a file,
applied by reading the wet file at the shifted offset; ``frac`` is reported and never applied.
"""
from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor as T

from . import _hip

MAX_LAG = 8192                                  # the L limit of mx_pair_xcorr


class PairLag(NamedTuple):
    """What ``estimate_pair_lag`` returns: (B,) device tensors, ``lag`` int32 (samples), ``frac`` fp32 (the parabolic
    sub-sample offset of the peak, in -0.5 .. 0.5, 0 at the window's edges) and ``corr`` fp32 (the normalised correlation at
    ``lag``, signed: its sign is the polarity)."""
    lag: T
    frac: T
    corr: T


def _rows(x: T, name: str, fn: str) -> T:
    """(B, N) view of an fp32 device tensor of shape (B, N), (B, 1, N) or (N,), rows a row stride apart left in place."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.ndim not in (1, 2, 3) or (x.ndim == 3 and x.size(1) != 1):
        raise ValueError(f"{fn}: {name} must be an fp32 tensor of shape (B, N), (B, 1, N) or (N,)")
    if not x.is_cuda:
        raise ValueError(f"{fn}: {name} must be on a HIP device (there is no CPU fallback)")
    x = x.detach()
    x = x.unsqueeze(0) if x.ndim == 1 else (x[:, 0, :] if x.ndim == 3 else x)
    B, N = x.shape
    if B == 0 or N == 0:
        raise ValueError(f"{fn}: {name} has no rows or no samples")
    if x.stride(1) != 1 or (B > 1 and x.stride(0) < N):
        x = x.contiguous()
    return x


def _stride(x: T) -> int:
    return max(x.stride(0), x.size(1)) if x.size(0) > 1 else x.size(1)


def _pair(dry: T, wet: T, max_lag, fn: str) -> Tuple[T, T, int]:
    d, w = _rows(dry, "dry", fn), _rows(wet, "wet", fn)
    if d.shape != w.shape or d.device != w.device:
        raise ValueError(f"{fn}: dry and wet must have the same rows on the same device, got {tuple(d.shape)} and {tuple(w.shape)}")
    top = min(MAX_LAG, d.size(1) - 1)
    if isinstance(max_lag, bool) or not isinstance(max_lag, int) or not 0 <= max_lag <= top:
        raise ValueError(f"{fn}: max_lag must be an int in 0 .. min({MAX_LAG}, N - 1) = {top}, got {max_lag!r}")
    return d, w, max_lag


def _xcorr(d: T, w: T, L: int) -> T:
    B, N = d.shape
    r = torch.empty((B, 2 * L + 1), device=d.device, dtype=torch.float64)
    _hip.call("mx_pair_xcorr", d.data_ptr(), _stride(d), w.data_ptr(), _stride(w), B, N, L, _hip.ptr(r), _hip.stream())
    return r


def xcorr_lags(dry: T, wet: T, max_lag: int) -> T:
    """(B, 2 max_lag + 1) fp64: ``r[b, l + max_lag] = sum_n dry[b, n] wet[b, n + l]`` (one ``mx_pair_xcorr`` launch)."""
    d, w, L = _pair(dry, wet, max_lag, "xcorr_lags")
    return _xcorr(d, w, L)


def estimate_pair_lag(dry: T, wet: T, max_lag: int) -> PairLag:
    """Lag, sub-sample offset and signed correlation of every row pair, searched over -max_lag .. max_lag, in two launches
    (``mx_pair_xcorr``, ``mx_pair_peak``).  ``dry`` and ``wet`` are fp32 on the device, (B, N), (B, 1, N) or (N,), with
    0 <= max_lag <= min(8192, N - 1); rows a row stride apart (inner stride 1) are read in place.  A row whose dry or wet is
    all zeros gets lag 0, corr 0, frac 0."""
    d, w, L = _pair(dry, wet, max_lag, "estimate_pair_lag")
    B, N = d.shape
    r = _xcorr(d, w, L)
    lag = torch.empty(B, device=d.device, dtype=torch.int32)
    corr = torch.empty(B, device=d.device, dtype=torch.float32)
    frac = torch.empty(B, device=d.device, dtype=torch.float32)
    _hip.call("mx_pair_peak", d.data_ptr(), _stride(d), w.data_ptr(), _stride(w), _hip.ptr(r), B, N, L, _hip.ptr(lag),
              _hip.ptr(corr), _hip.ptr(frac), _hip.stream())
    return PairLag(lag, frac, corr)


def shift_rows(wet: T, lag: T, corr: Optional[T] = None, out: Optional[T] = None) -> T:
    """``out[b, n] = s_b * wet[b, n + lag[b]]``, 0 where ``n + lag[b]`` leaves the row; ``s_b = -1`` where ``corr[b] < 0``,
    else +1 (``corr=None``: no polarity).  ``lag`` is (B,) int32 and ``corr`` (B,) fp32, on ``wet``'s device.  The result has
    ``wet``'s shape; a given ``out`` (fp32, that shape, inner stride 1, rows at least N apart) is written in place -- it may
    be a strided view, and it may not overlap ``wet``."""
    fn = "shift_rows"
    w = _rows(wet, "wet", fn)
    B, N = w.shape
    if not isinstance(lag, torch.Tensor) or lag.dtype != torch.int32 or lag.shape != (B,) or lag.device != w.device:
        raise ValueError(f"{fn}: lag must be an int32 tensor of shape ({B},) on wet's device")
    if corr is not None and (not isinstance(corr, torch.Tensor) or corr.dtype != torch.float32 or corr.shape != (B,)
                             or corr.device != w.device):
        raise ValueError(f"{fn}: corr must be an fp32 tensor of shape ({B},) on wet's device, or None")
    if out is None:
        out = torch.empty(wet.shape, device=w.device, dtype=torch.float32)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.shape != wet.shape
          or out.device != w.device):
        raise ValueError(f"{fn}: out must be an fp32 tensor of wet's shape {tuple(wet.shape)} on wet's device")
    o = out.unsqueeze(0) if out.ndim == 1 else (out[:, 0, :] if out.ndim == 3 else out)
    if o.stride(1) != 1 or (B > 1 and o.stride(0) < N):
        raise ValueError(f"{fn}: out needs inner stride 1 and rows at least N = {N} floats apart")
    lo, hi = o.data_ptr(), o.data_ptr() + 4 * ((B - 1) * _stride(o) + N)
    if lo < w.data_ptr() + 4 * ((B - 1) * _stride(w) + N) and w.data_ptr() < hi:
        raise ValueError(f"{fn}: out may not overlap wet")
    _hip.call("mx_pair_shift", w.data_ptr(), _stride(w), B, N, _hip.ptr(lag.contiguous()),
              None if corr is None else _hip.ptr(corr.contiguous()), o.data_ptr(), _stride(o), _hip.stream())
    return out


def align_pairs(dry: T, wet: T, max_lag: int) -> Tuple[T, PairLag]:
    """(wet_aligned, PairLag) for a device batch: ``estimate_pair_lag`` and ``shift_rows`` with its lag and polarity, so
    that ``wet_aligned ~ dry`` row by row (three launches).  Every ROW gets its own lag; the data path estimates one lag
    a FILE instead (``datasets.RandomAudioChunkDryWetDataset.estimate_alignment``) and shifts by reading the file."""
    est = estimate_pair_lag(dry, wet, max_lag)
    return shift_rows(wet, est.lag, est.corr), est

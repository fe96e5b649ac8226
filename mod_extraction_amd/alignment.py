"""K19: the constant lag and the polarity of recorded dry / wet pairs, by cross-correlation on the device
(csrc/pair_align.hip; include/modex_hip.h, K19, has the definition) -- no counterpart in the reference.

    r[b, l + L] = sum_n dry[b, n] wet[b, n + l],  l = -L..L;   c = r / sqrt(sum dry^2 sum wet^2)
    lag = argmax |c| (ties: smallest |l|, then l >= 0);  corr = c[lag];  frac = the parabolic sub-sample offset

Convention: ``wet[n + lag] ~ sign(corr) * dry[n]``: a wet that is late by d samples has ``lag = +d``, and
``shift_rows(wet, lag, corr)`` lines it up with ``dry``.  Everything here returns device tensors and never synchronises with
the host.  ``datasets.RandomAudioChunkDryWetDataset.estimate_alignment`` is the user of the estimate: one integer lag a file,
applied by reading the wet file at the shifted offset; ``frac`` is reported and never applied there.

K26 (csrc/warp.hip; csrc/warp_abi.h has the definition): a wet recorded on another clock than its dry lies on a LINE of lags,
``wet[offset + (1 + drift) n] ~ polarity * dry[n]``.  ``estimate_file_drift`` finds the line from K19's estimate on short probes
(``lag + frac``, a Theil-Sen fit on the host: ``fit_lag_line``), ``warp_rows`` reads rows along such a line on the device, and
``warp_tree`` puts a directory of wet files on their dry files' time base, once, on disk.
"""
import logging
import os
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor as T

from . import _hip

log = logging.getLogger(__name__)
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


# ---- K26: two clocks -- a straight line of lags over the file, and the warp that undoes it ---------------------------------
MAX_DRIFT = _hip.WARP_MAX_DRIFT                 # MX_WARP_MAX_DRIFT
MAX_OFFSET = _hip.WARP_MAX_OFFSET               # MX_WARP_MAX_OFFSET
WARP_STAMP_SUFFIX = ".warped.json"


class PairDrift(NamedTuple):
    """One file pair's line of lags, host numbers: ``wet[offset + (1 + drift) n] ~ polarity * dry[n]`` -- ``offset`` in samples
    at sample 0, ``drift`` the clock ratio minus one (1e-6 is 1 ppm); ``drift = 0`` with an integer ``offset`` is K19's
    ``lag``.  ``corr``: the median |corr| of all probes; ``resid``: the largest miss, in samples, of a probe the line was
    fitted through (0 where none was fitted); ``n_probes``: how many it was fitted through; ``ok`` False where the estimate
    is not trusted -- then offset 0, drift 0, polarity +1."""
    offset: float
    drift: float
    polarity: int
    corr: float
    resid: float
    n_probes: int
    ok: bool


def fit_lag_line(centres: Sequence[float], lags: Sequence[float], corrs: Sequence[float], min_corr: float = 0.5,
                 max_resid: float = 0.5, min_probes: int = 3) -> PairDrift:
    """The line ``lag = offset + drift * centre`` through a file's probes, in host fp64 (no device): probes with ``corr == 0``
    or ``|corr| < min_corr`` are left out; Theil-Sen on the rest -- ``drift`` is the median of the slopes of every two probes
    at different centres, ``offset`` the median of ``lag - drift * centre`` (so it refers to sample 0).  Periodic material
    puts single probes a period off; the two medians outvote them, and they still show in ``resid``, the largest
    ``|lag - line|`` of a probe that was not left out.  ``polarity``: the sign of those probes' summed corr.  Not trusted
    (``ok`` False, offset 0, drift 0, polarity +1), tested in this order: fewer than ``min_probes`` probes are left, or no
    two of them at different centres; the median |corr| of ALL probes is below ``min_corr``; ``resid > max_resid``."""
    c, l, r = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (centres, lags, corrs))
    if not (c.size == l.size == r.size):
        raise ValueError("fit_lag_line: one centre, one lag and one corr per probe")
    if isinstance(min_probes, bool) or not isinstance(min_probes, int) or min_probes < 2:
        raise ValueError(f"fit_lag_line: min_probes must be an int >= 2, got {min_probes!r}")
    if not 0.0 <= min_corr <= 1.0 or not max_resid >= 0.0:
        raise ValueError("fit_lag_line: min_corr must be in 0 .. 1 and max_resid >= 0")
    med = float(np.median(np.abs(r))) if r.size else 0.0
    keep = (r != 0.0) & (np.abs(r) >= min_corr)
    c, l, r = c[keep], l[keep], r[keep]
    n = int(c.size)
    i, j = np.triu_indices(n, 1)
    apart = c[i] != c[j]
    if n < min_probes or not bool(apart.any()):
        return PairDrift(0.0, 0.0, 1, med, 0.0, n, False)
    drift = float(np.median((l[j][apart] - l[i][apart]) / (c[j][apart] - c[i][apart])))
    offset = float(np.median(l - drift * c))
    resid = float(np.max(np.abs(l - (offset + drift * c))))
    if not med >= min_corr or not resid <= max_resid:
        return PairDrift(0.0, 0.0, 1, med, resid, n, False)
    return PairDrift(offset, drift, -1 if float(np.sum(r)) < 0.0 else 1, med, resid, n, True)


def _pos_int(v, name: str, fn: str, lo: int = 1) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or v < lo:
        raise ValueError(f"{fn}: {name} must be an int >= {lo}, got {v!r}")
    return v


def probe_starts(n_dry: int, n_wet: int, probe_points: int, n_probes: int) -> Tuple[int, int]:
    """(hop, span) of ``estimate_file_drift``'s probes: ``n_probes`` starts ``k * hop``, ``hop = span // (n_probes - 1)``,
    over ``span = min(n_dry, n_wet) - probe_points`` (a ValueError when that is negative)."""
    span = min(n_dry, n_wet) - probe_points
    if span < 0:
        raise ValueError(f"estimate_file_drift: files of {n_dry} and {n_wet} samples are shorter than one probe of {probe_points}")
    return span // (n_probes - 1), span


def estimate_file_drift(dry: T, wet: T, max_lag: int, probe_points: int = 8192, n_probes: int = 16, min_corr: float = 0.5,
                        max_resid: float = 0.5, min_probes: int = 3) -> PairDrift:
    """The ``PairDrift`` of one recording: ``dry`` (L_d,) and ``wet`` (L_w,) fp32 on the device, of any two lengths.
    ``n_probes`` probes of ``probe_points`` samples start ``hop = (min(L_d, L_w) - probe_points) // (n_probes - 1)`` apart from
    sample 0 in both files -- strided views of the two rows where ``hop >= probe_points`` (no copy), gathered rows otherwise;
    one ``estimate_pair_lag`` call (K19's two kernels as they are) gives every probe's lag, ``frac`` and corr, one ``.cpu()``
    brings them to the host, and ``fit_lag_line`` fits ``lag + frac`` at ``centre = start + (probe_points - 1) / 2``.

    Reach: a probe sees lags up to ``max_lag``, so the line must stay inside it over the file: ``|offset| + |drift| L <=
    max_lag <= min(8192, probe_points - 1)``.  Within one probe the lag moves by ``|drift| probe_points`` samples, which
    smears the probe's own peak: keep that well under a sample (8192 points at 100 ppm move 0.8; the 22 272-point probes of
    ``estimate_alignment`` are too long for this).  ``frac`` is a parabola through three points of |c|: biased on narrow-band
    material.  Checks, in this order: ``max_lag``, ``probe_points``, ``n_probes`` (ints; n_probes >= 2, probe_points >= 2,
    0 <= max_lag <= min(8192, probe_points - 1)); ``fit_lag_line``'s three; ``dry`` then ``wet`` (fp32, one dimension); both
    at least ``probe_points`` long; both on one HIP device."""
    fn = "estimate_file_drift"
    L = _pos_int(max_lag, "max_lag", fn, 0)
    P, K = _pos_int(probe_points, "probe_points", fn, 2), _pos_int(n_probes, "n_probes", fn, 2)
    if L > min(MAX_LAG, P - 1):
        raise ValueError(f"{fn}: max_lag must be in 0 .. min({MAX_LAG}, probe_points - 1) = {min(MAX_LAG, P - 1)}, got {L}")
    fit_lag_line([], [], [], min_corr, max_resid, min_probes)                  # its argument checks
    for name, v in (("dry", dry), ("wet", wet)):
        if not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or v.ndim != 1:
            raise ValueError(f"{fn}: {name} must be an fp32 tensor of shape (L,)")
    hop, _ = probe_starts(dry.numel(), wet.numel(), P, K)
    if not dry.is_cuda or dry.device != wet.device:
        raise ValueError(f"{fn}: dry and wet must be on one HIP device (there is no CPU fallback)")
    d, w = dry.detach().contiguous(), wet.detach().contiguous()
    if hop >= P:
        dp, wp = d.as_strided((K, P), (hop, 1)), w.as_strided((K, P), (hop, 1))
    else:
        idx = (torch.arange(K, device=d.device) * hop)[:, None] + torch.arange(P, device=d.device)[None, :]
        dp, wp = d[idx], w[idx]
    est = estimate_pair_lag(dp, wp, L)
    table = torch.stack([est.lag.double(), est.frac.double(), est.corr.double()]).cpu().numpy()
    centres = np.arange(K, dtype=np.float64) * hop + (P - 1) / 2.0
    return fit_lag_line(centres, table[0] + table[1], table[2], min_corr, max_resid, min_probes)


def _lib_warp_plan(fn: str, zeros: int, rolloff: float, beta: float, n_in: int, n_out: int, drift_bound: float,
                   offset_bound: float) -> Tuple[int, int, int, int]:
    """(half, taps, tiles, span) of ``mx_warp_plan``; its refusals as ValueErrors."""
    import ctypes
    i32 = (ctypes.c_int32 * 3)()
    i64 = (ctypes.c_int64 * 1)()
    a32 = ctypes.addressof(i32)
    rc = _hip.load().mx_warp_plan(zeros, rolloff, beta, n_in, n_out, drift_bound, offset_bound, a32, a32 + 4,
                                  ctypes.addressof(i64), a32 + 8)
    if rc == -2:
        raise ValueError(f"{fn}: beyond the warp's limits (|drift| <= {MAX_DRIFT}, |offset| < 2^31, at most 4095 taps, beta <= "
                         f"64, rows of at most 2^40 samples): zeros = {zeros}, rolloff = {rolloff}, beta = {beta}, n = {n_in} -> "
                         f"{n_out}, |drift| <= {drift_bound}, |offset| <= {offset_bound}")
    if rc != 0:
        raise ValueError(f"{fn}: need zeros, n_in, n_out >= 1, 0 < rolloff <= 1, beta >= 0 and finite offset and drift; got zeros "
                         f"= {zeros}, rolloff = {rolloff}, beta = {beta}, n = {n_in} -> {n_out}, |drift| <= {drift_bound}, "
                         f"|offset| <= {offset_bound}")
    return i32[0], i32[1], i64[0], i32[2]


def warp_plan(n_in: int, n_out: int, zeros: int = 48, rolloff: float = 0.95, beta: float = 16.0, max_drift: float = 0.0,
              max_offset: float = 0.0) -> Tuple[int, int, int, int]:
    """(half, taps, tiles, span) of a warp of rows of ``n_in`` samples onto ``n_out``: the library's host arithmetic
    (``mx_warp_plan``), a ValueError beyond its limits."""
    fn = "warp_plan"
    return _lib_warp_plan(fn, _pos_int(zeros, "zeros", fn), float(rolloff), float(beta), _pos_int(n_in, "n_in", fn),
                          _pos_int(n_out, "n_out", fn), float(max_drift), float(max_offset))


def warp_rows(x: T, offset, drift, n_out: Optional[int] = None, polarity=None, out: Optional[T] = None, zeros: int = 48,
              rolloff: float = 0.95, beta: float = 16.0) -> T:
    """``out[b, m] = s_b * x_b(m + (m * drift[b] + offset[b]))``: every row of ``x`` read along its own straight line by a
    Kaiser-windowed sinc evaluated at each output's own fractional position (csrc/warp_abi.h has the definition), in one
    ``mx_warp_rows`` launch per 65535 rows and without a host synchronisation.  With a ``PairDrift`` ``p`` of (dry, wet),
    ``warp_rows(wet, p.offset, p.drift, n_out=len(dry), polarity=p.polarity) ~ dry``'s time base.

    ``x``: (B, n) or (n,) fp32 on the device, rows any row stride apart (inner stride 1) read in place.  ``offset``, ``drift``:
    floats, or (B,) fp64 tensors on ``x``'s device; floats beyond ``|drift| <= 1e-3`` / ``|offset| < 2^31`` are a ValueError,
    and a row whose device values are beyond them comes back as NaNs.  ``n_out`` defaults to n.  ``polarity``: None, +1 / -1,
    or a (B,) fp32 tensor whose negative entries invert their row (K19's ``corr`` serves).  ``out``: an fp32 tensor of the
    result's shape on the same device, inner stride 1, any row stride; it must not share memory with ``x`` or the parameter
    tensors.  A warp is not a shift: it low-passes above ``rolloff`` times Nyquist even at drift 0 (``shift_rows`` is exact).
    Checks, in this order: ``x``; ``zeros``, ``rolloff``, ``beta``, ``n_out`` and float ``offset`` / ``drift`` (by
    ``mx_warp_plan``); tensor ``offset`` / ``drift``; ``polarity``; ``out``; ``x`` on a HIP device."""
    fn = "warp_rows"
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.ndim not in (1, 2):
        raise ValueError(f"{fn}: x must be an fp32 tensor of shape (B, n) or (n,)")
    rows = x.detach() if x.ndim == 2 else x.detach().unsqueeze(0)
    B, n = rows.shape
    if B < 1 or n < 1:
        raise ValueError(f"{fn}: need at least one row of at least one sample, got {tuple(x.shape)}")
    if rows.stride(1) != 1 and n > 1:
        raise ValueError(f"{fn}: the samples of a row must be contiguous (inner stride 1), got strides {tuple(x.stride())}")
    x_stride = rows.stride(0) if B > 1 else n
    if x_stride < n:
        raise ValueError(f"{fn}: rows of x overlap (row stride {x_stride} < n = {n})")
    n_out = n if n_out is None else _pos_int(n_out, "n_out", fn)
    params = {}
    for name, v in (("offset", offset), ("drift", drift)):
        if isinstance(v, torch.Tensor):
            params[name] = None
        elif isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
            raise ValueError(f"{fn}: {name} must be a float or a ({B},) fp64 tensor, got {v!r}")
        else:
            params[name] = abs(float(v))
    _lib_warp_plan(fn, _pos_int(zeros, "zeros", fn), float(rolloff), float(beta), n, n_out, params["drift"] or 0.0,
                   params["offset"] or 0.0)
    dev_params = []
    for name, v in (("offset", offset), ("drift", drift)):
        if isinstance(v, torch.Tensor):
            if v.dtype != torch.float64 or v.shape != (B,) or v.device != x.device:
                raise ValueError(f"{fn}: {name} must be a float or a ({B},) fp64 tensor on x's device")
            dev_params.append(v.detach().contiguous())
        else:
            dev_params.append(None)
    sign = None
    if isinstance(polarity, torch.Tensor):
        if polarity.dtype != torch.float32 or polarity.shape != (B,) or polarity.device != x.device:
            raise ValueError(f"{fn}: polarity must be None, +1, -1 or a ({B},) fp32 tensor on x's device")
        sign = polarity.detach().contiguous()
    elif polarity is not None and (isinstance(polarity, bool) or polarity not in (1, -1)):
        raise ValueError(f"{fn}: polarity must be None, +1, -1 or a ({B},) fp32 tensor on x's device, got {polarity!r}")
    shape = (B, n_out) if x.ndim == 2 else (n_out,)
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != shape
                            or out.device != x.device):
        raise ValueError(f"{fn}: out must be an fp32 tensor of shape {shape} on x's device")
    if out is not None:
        orows = out.detach() if out.ndim == 2 else out.detach().unsqueeze(0)
        if orows.stride(1) != 1 and n_out > 1:
            raise ValueError(f"{fn}: the samples of a row of out must be contiguous (inner stride 1), got strides {tuple(out.stride())}")
        if B > 1 and orows.stride(0) < n_out:
            raise ValueError(f"{fn}: rows of out overlap (row stride {orows.stride(0)} < n_out = {n_out})")
        lo, hi = orows.data_ptr(), orows.data_ptr() + 4 * ((B - 1) * orows.stride(0) + n_out if B > 1 else n_out)
        others = [(rows.data_ptr(), rows.data_ptr() + 4 * ((B - 1) * x_stride + n))]
        others += [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in (*dev_params, sign) if t is not None]
        if any(lo < b and a < hi for a, b in others):
            raise ValueError(f"{fn}: out may not overlap x, offset, drift or polarity")
    if not x.is_cuda:
        raise ValueError(f"{fn}: x must be on a HIP device (there is no CPU fallback)")
    with torch.cuda.device(x.device):
        if out is None:
            out = torch.empty(shape, device=x.device, dtype=torch.float32)
            orows = out if out.ndim == 2 else out.unsqueeze(0)
        for i, v in enumerate((offset, drift)):
            if dev_params[i] is None:
                dev_params[i] = torch.full((B,), float(v), device=x.device, dtype=torch.float64)
        if sign is None and polarity == -1:
            sign = torch.full((B,), -1.0, device=x.device, dtype=torch.float32)
        _hip.call("mx_warp_rows", rows.data_ptr(), x_stride, B, n, _hip.ptr(dev_params[0]), _hip.ptr(dev_params[1]),
                  _hip.ptr(sign), zeros, float(rolloff), float(beta), orows.data_ptr(), orows.stride(0) if B > 1 else n_out, n_out,
                  _hip.stream())
    return out


# ---- a directory of recorded pairs -----------------------------------------------------------------------------------------
def _file_stamp(path: str) -> Dict[str, int]:
    st = os.stat(path)
    return {"size": st.st_size, "mtime_ns": st.st_mtime_ns}


def warp_tree(dry_dir: str, wet_dir: str, dst_dir: str, sr: int, max_lag: int, ext: str = "wav", device="cuda",
              min_drift_samples: float = 0.25, probe_points: int = 8192, n_probes: int = 16, min_corr: float = 0.5,
              max_resid: float = 0.5, min_probes: int = 3, zeros: int = 48, rolloff: float = 0.95,
              beta: float = 16.0) -> Dict[str, PairDrift]:
    """Every ``*ext`` file under ``wet_dir`` put on the time base of the file at the same relative path under ``dry_dir``, and
    written under that path in ``dst_dir``: ``{relative path: PairDrift}``.  The datasets cut their items at integer offsets
    from files, so drift is undone once, on disk, as ``resample.convert_tree`` does for the rate.

    Per pair: ``estimate_file_drift`` on channel 0 of the two files (``max_lag`` in samples and the probe settings as there),
    then one of three routes, recorded in the stamp's ``route``:
      "warp"   ``warp_rows`` on all channels along the estimated line: the result has the DRY's frame count, the polarity is
               applied, and the dataset's own K19 estimate on it finds lag 0 and polarity +1;
      "shift"  ``|drift| * frames < min_drift_samples``: the two files share a clock.  K19's exact path -- ``shift_rows`` by
               ``round(offset)`` and the polarity, cut or zero-padded to the dry's frame count: no interpolation, the wet's
               own samples bit for bit (a warp would low-pass them above ``rolloff`` times Nyquist);
      "copy"   the estimate is not trusted, or the two files differ in rate or channels, are not at ``sr`` or are shorter
               than a probe: the wet is copied byte for byte, its ``PairDrift`` has ``ok`` False, and all such pairs are
               named in one warning.
    A dry file without a wet file is a ValueError.  Files appear by ``os.replace`` of a temporary file, float32 RIFF; a stamp
    ``<file>.warped.json`` records both sources' size and mtime, the settings and the estimate, and a pair whose stamp still
    matches is skipped: a second run converts nothing and returns the same table.  The conversion is deterministic, so the
    ranks of a distributed run that race on one file write the same bytes."""
    import json
    import shutil
    from . import datasets
    from .resample import _read_stamp, _replace_into
    fn = "warp_tree"
    sr, L = _pos_int(sr, "sr", fn), _pos_int(max_lag, "max_lag", fn, 0)
    P, K = _pos_int(probe_points, "probe_points", fn, 2), _pos_int(n_probes, "n_probes", fn, 2)
    if L > min(MAX_LAG, P - 1):
        raise ValueError(f"{fn}: max_lag must be in 0 .. min({MAX_LAG}, probe_points - 1) = {min(MAX_LAG, P - 1)}, got {L}")
    if not min_drift_samples >= 0.0:
        raise ValueError(f"{fn}: min_drift_samples must be >= 0, got {min_drift_samples!r}")
    fit_lag_line([], [], [], min_corr, max_resid, min_probes)
    _lib_warp_plan(fn, _pos_int(zeros, "zeros", fn), float(rolloff), float(beta), 1, 1, 0.0, 0.0)
    if len({os.path.abspath(d) for d in (dry_dir, wet_dir, dst_dir)}) != 3:
        raise ValueError(f"{fn}: dry_dir, wet_dir and dst_dir must be three directories")
    settings = {"sr": sr, "max_lag": L, "probe_points": P, "n_probes": K, "min_corr": float(min_corr),
                "max_resid": float(max_resid), "min_probes": int(min_probes), "min_drift_samples": float(min_drift_samples),
                "filter": [int(zeros), float(rolloff), float(beta)]}
    done: Dict[str, PairDrift] = {}
    routes = {"warp": 0, "shift": 0, "copy": 0, "kept": 0}
    bad = []
    for dry_p in datasets.list_files(dry_dir, ext):
        rel = os.path.relpath(dry_p, dry_dir)
        wet_p, dst = os.path.join(wet_dir, rel), os.path.join(dst_dir, rel)
        if not os.path.isfile(wet_p):
            raise ValueError(f"{fn}: no wet file for {rel} under {wet_dir}")
        stamp = dict(settings, dry=_file_stamp(dry_p), wet=_file_stamp(wet_p))
        old = _read_stamp(dst + WARP_STAMP_SUFFIX)
        if old is not None and os.path.isfile(dst) and all(old.get(k) == v for k, v in stamp.items()):
            done[rel] = PairDrift(*old["estimate"])
            routes["kept"] += 1
            if not done[rel].ok:
                bad.append(rel)
            continue
        os.makedirs(os.path.dirname(dst) or ".", exist_ok=True)
        (d_frames, d_sr, d_ch), (w_frames, w_sr, w_ch) = datasets.wav_info(dry_p), datasets.wav_info(wet_p)
        est, route = PairDrift(0.0, 0.0, 1, 0.0, 0.0, 0, False), "copy"
        if d_sr == w_sr == sr and d_ch == w_ch and min(d_frames, w_frames) >= P:
            dry = datasets.wav_load(dry_p)[0][0].to(device)
            wet = datasets.wav_load(wet_p)[0].to(device)                    # (channels, frames)
            est = estimate_file_drift(dry, wet[0], L, P, K, min_corr, max_resid, min_probes)
            if est.ok and abs(est.drift) * d_frames < min_drift_samples:
                route = "shift"
                n = max(d_frames, w_frames)
                padded = torch.zeros((w_ch, n), device=wet.device, dtype=torch.float32)
                padded[:, :w_frames] = wet
                lag = torch.full((w_ch,), int(round(est.offset)), dtype=torch.int32, device=wet.device)
                sign = torch.full((w_ch,), float(est.polarity), dtype=torch.float32, device=wet.device)
                y = shift_rows(padded, lag, sign)[:, :d_frames].cpu()
            elif est.ok:
                route = "warp"
                y = warp_rows(wet, est.offset, est.drift, n_out=d_frames, polarity=est.polarity, zeros=zeros, rolloff=rolloff,
                              beta=beta).cpu()
        if route == "copy":
            bad.append(rel)
            _replace_into(dst, lambda tmp: shutil.copyfile(wet_p, tmp))
        else:
            _replace_into(dst, lambda tmp: datasets.wav_save(tmp, y, sr))
        routes[route] += 1
        stamp.update(estimate=list(est), route=route)

        def write_stamp(tmp: str) -> None:
            with open(tmp, "w") as f:
                json.dump(stamp, f, sort_keys=True)

        _replace_into(dst + WARP_STAMP_SUFFIX, write_stamp)
        done[rel] = est
    if bad:
        log.warning("drift estimate not trusted (too few probes, median |corr| < %.2f, a probe more than %.2f samples off the "
                    "line, or files that do not match), wet copied as it is: %s", min_corr, max_resid, ", ".join(bad))
    log.info("%s on %s -> %s: %d warped, %d shifted, %d copied, %d already there", wet_dir, dry_dir, dst_dir, routes["warp"],
             routes["shift"], routes["copy"], routes["kept"])
    return done


def summarise_drift(table: Dict[str, PairDrift]) -> str:
    """One line on a ``warp_tree`` table: files, trusted, the range of drift in ppm and of offset in samples, inverted."""
    good = [p for p in table.values() if p.ok]
    ppm = [1e6 * p.drift for p in good] or [0.0]
    off = [p.offset for p in good] or [0.0]
    return (f"{len(table)} files, {len(good)} trusted, drift {min(ppm):.1f} .. {max(ppm):.1f} ppm, offset {min(off):.1f} .. "
            f"{max(off):.1f} samples, {sum(p.polarity < 0 for p in good)} inverted")

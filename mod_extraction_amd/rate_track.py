"""The rate contour of an LFO track whose rate moves (K25, csrc/rate_track.hip; csrc/rate_track_abi.h has the definition) -- no
counterpart in the reference.

    fit_rate_track         a track cut into slices: K18's candidates per slice, a Viterbi path per shape that joins one candidate
                           a slice by rate and phase continuity, one shape per row, K18's refinement per slice
    rate_track_plan        (S, K) of such a fit: host arithmetic with the library's formula
    synth_from_rate_track  the slices' templates joined by K22's taper: the clean LFO the contour describes
    rate_at                the slice centres in seconds and the rates there

Device tensors throughout; nothing here synchronises with the host.
"""
import ctypes
import math
from typing import NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor as T

from . import _hip
from .modulations import LFO_SHAPES, LFOFit, _fl32, fit_rate_window, fit_shape_mask, synth_from_fit

_LIM = _hip.RATE_TRACK_LIMITS                   # the MX_RATE_TRACK_* numbers of csrc/rate_track_abi.h
RATE_TRACK_MIN_SLICE, RATE_TRACK_MAX_SLICE = _LIM["MIN_W"], _LIM["MAX_W"]
RATE_TRACK_MAX_SLICES = _LIM["MAX_S"]
RATE_TRACK_MAX_STATES = _LIM["MAX_STATES"]      # K * n_phases, the states of a slice
RATE_TRACK_MAX_STEP = _LIM["MAX_D"]
RATE_TRACK_MAX_ROWS = _LIM["MAX_ROWS"]
RATE_TRACK_MAX_POINTS = _LIM["MAX_N"]


class RateTrack(NamedTuple):
    """What ``fit_rate_track`` returns.  ``shape`` (B,) int32 (ids of ``modulations.SHAPE_IDS``): one shape a row; ``grid_k``,
    ``grid_j`` (B, S) int32: the path over the coarse grid; ``rate_hz``, ``phase``, ``amp``, ``offset``, ``resid`` (B, S) fp32: the
    refined fit of every slice -- ``offset + amp * make_mod_signals(slice_points, sr, rate_hz, phase, shape)`` is the slice's
    template; ``cost`` (B,) and ``per_shape_cost`` (B, 7) fp32 (+inf where a shape was not allowed): the total path costs;
    ``starts`` (S,) int64: the first point of every slice; the ints ``slice_points`` and ``n_points``; ``sr``, the point rate the
    fit was given (a float: ``synth_from_rate_track`` needs it)."""
    shape: T
    grid_k: T
    grid_j: T
    rate_hz: T
    phase: T
    amp: T
    offset: T
    resid: T
    cost: T
    per_shape_cost: T
    starts: T
    slice_points: int
    n_points: int
    sr: float


def _pos_int(v, name: str) -> int:
    if isinstance(v, bool) or not isinstance(v, int):
        raise ValueError(f"fit_rate_track: {name} must be an int, got {v!r}")
    return v


def rate_track_plan(n: int, sr: float, slice_points: int, hop_points: Optional[int] = None, rate_hz=(0.25, 8.0),
                    rate_div: int = 4, n_phases: int = 32) -> Tuple[int, int]:
    """(S, K): the slices ``file_eval.window_starts(n, slice_points, hop_points)`` cuts (hop defaults to half a slice) and the
    rates of a slice's grid, K = floor((f_max - f_min) / df) + 1, df = 1 / (rate_div (slice_points / sr)) in fp64 on the fp32
    roundings of the window and of sr -- ``mx_rate_track_plan``'s formula.  Pure host arithmetic; what the library would refuse
    is a ValueError."""
    from .file_eval import window_starts
    fn = "fit_rate_track"
    n, W = _pos_int(n, "the number of points"), _pos_int(slice_points, "slice_points")
    f_min, f_max = fit_rate_window(rate_hz, float(sr))
    if not RATE_TRACK_MIN_SLICE <= W <= RATE_TRACK_MAX_SLICE:
        raise ValueError(f"{fn}: slice_points must be in {RATE_TRACK_MIN_SLICE} .. {RATE_TRACK_MAX_SLICE}, got {W}")
    if not W <= n <= RATE_TRACK_MAX_POINTS:
        raise ValueError(f"{fn}: rows of {n} points; need slice_points = {W} <= n <= {RATE_TRACK_MAX_POINTS}")
    rate_div, J = _pos_int(rate_div, "rate_div"), _pos_int(n_phases, "n_phases")
    if not 1 <= rate_div <= 16:
        raise ValueError(f"{fn}: rate_div must be in 1 .. 16, got {rate_div}")
    if not 4 <= J <= 128:
        raise ValueError(f"{fn}: n_phases must be in 4 .. 128, got {J}")
    hop = max(1, W // 2) if hop_points is None else _pos_int(hop_points, "hop_points")
    if not 1 <= hop <= W:
        raise ValueError(f"{fn}: hop_points must be in 1 .. slice_points = {W}, got {hop}")
    S = len(window_starts(n, W, hop))
    if S > RATE_TRACK_MAX_SLICES:
        raise ValueError(f"{fn}: {S} slices; the path takes at most {RATE_TRACK_MAX_SLICES} (a larger hop)")
    df = 1.0 / (rate_div * (W / _fl32(float(sr))))
    K = int(math.floor((_fl32(f_max) - _fl32(f_min)) / df)) + 1
    if K * J > RATE_TRACK_MAX_STATES:
        raise ValueError(f"{fn}: the rate window {rate_hz!r} needs {K} rates x {J} phases on {W} points at rate_div = {rate_div}; "
                         f"a slice takes at most {RATE_TRACK_MAX_STATES} states")
    return S, K


def fit_rate_track(mod_sig: T, sr: float, slice_points: int, hop_points: Optional[int] = None, rate_hz=(0.25, 8.0),
                   shapes: Sequence[str] = LFO_SHAPES, rate_div: int = 4, n_phases: int = 32, n_rounds: int = 4,
                   max_rate_step: int = 2, rate_weight: float = 0.002, phase_weight: float = 1.0) -> RateTrack:
    """The rate contour of every row of ``mod_sig`` ((B, n) or (n,), fp32, on the device; ``sr`` the rate of its points).  The row
    is cut into slices of ``slice_points`` points every ``hop_points`` (default half a slice; the last one right-aligned).  Every
    slice gets ``fit_lfo``'s coarse grid on ``slice_points`` points; per allowed shape a least-cost path takes one grid candidate
    a slice, a step costing ``rate_weight`` (bins moved)^2 + ``phase_weight`` (cycles by which the phase misses the advance of the
    mean rate over the hop)^2 and moving at most ``max_rate_step`` bins; the row's shape is the one whose path is cheapest, and
    ``n_rounds`` rounds of K18's refinement polish every slice from the path's candidate.  Rows a row stride apart (inner stride
    1) are read in place.  With ONE slice the result is ``fit_lfo``'s on that slice bit for bit only where K18 itself sums in
    ascending order (more than 512 grid candidates, ``K * n_phases > 512``) and where the coarse grid picks the shape the refined
    fit picks (always so with one allowed shape): the contour chooses its shape by the coarse path cost, ``fit_lfo`` by the
    refined residual, so on a small grid or on noisy rows with several shapes allowed the two may differ.  Four enqueues (``mx_rate_track_nodes`` / ``_path`` / ``_refine`` after the host-only
    ``mx_rate_track_plan``) with a node table and a workspace from ``torch.empty``."""
    from .file_eval import window_starts
    fn = "fit_rate_track"
    mask = fit_shape_mask(shapes)
    f_min, f_max = fit_rate_window(rate_hz, float(sr))
    if not isinstance(mod_sig, torch.Tensor) or mod_sig.ndim not in (1, 2) or mod_sig.dtype != torch.float32:
        raise ValueError(f"{fn}: mod_sig must be an fp32 tensor of shape (B, n) or (n,)")
    if not mod_sig.is_cuda:
        raise ValueError(f"{fn}: mod_sig must be on a HIP device (there is no CPU fallback)")
    m = mod_sig.detach()
    m = m.unsqueeze(0) if m.ndim == 1 else m
    B, n = m.shape
    if not 1 <= B <= RATE_TRACK_MAX_ROWS:
        raise ValueError(f"{fn}: mod_sig has {B} rows; need 1 .. {RATE_TRACK_MAX_ROWS}")
    W = _pos_int(slice_points, "slice_points")
    S, _ = rate_track_plan(n, sr, W, hop_points, (f_min, f_max), rate_div, n_phases)
    L, D = _pos_int(n_rounds, "n_rounds"), _pos_int(max_rate_step, "max_rate_step")
    if not 0 <= L <= 8:
        raise ValueError(f"{fn}: n_rounds must be in 0 .. 8, got {L}")
    if not 0 <= D <= RATE_TRACK_MAX_STEP:
        raise ValueError(f"{fn}: max_rate_step must be in 0 .. {RATE_TRACK_MAX_STEP}, got {D}")
    rw, pw = float(rate_weight), float(phase_weight)
    if not (0.0 <= rw < math.inf and 0.0 <= pw < math.inf):
        raise ValueError(f"{fn}: rate_weight and phase_weight must be finite and >= 0, got {rate_weight!r} and {phase_weight!r}")
    hop = max(1, W // 2) if hop_points is None else hop_points
    if m.stride(1) != 1 or (B > 1 and m.stride(0) < n):
        m = m.contiguous()
    stride = max(m.stride(0), n) if B > 1 else n
    dev = m.device
    starts = torch.tensor(window_starts(n, W, hop), dtype=torch.int64, device=dev)
    J = int(n_phases)
    grid = (f_min, f_max, mask, int(rate_div), J)
    sizes = (ctypes.c_int64 * 3)()                                      # K, the node table's and the workspace's bytes
    a = ctypes.addressof(sizes)
    _hip.call("mx_rate_track_plan", B, n, float(sr), S, W, *grid, L, D, a, a + 8, a + 16)
    node = torch.empty((sizes[1] + 7) // 8, device=dev, dtype=torch.float64)
    ws = torch.empty((sizes[2] + 7) // 8, device=dev, dtype=torch.float64)
    buffers = (node.data_ptr(), node.numel() * 8, ws.data_ptr(), ws.numel() * 8)
    i32 = lambda *s: torch.empty(s, device=dev, dtype=torch.int32)
    f32 = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)
    shape, grid_k, grid_j, cost, per_shape = i32(B), i32(B, S), i32(B, S), f32(B), f32(B, 7)
    fitted = [f32(B, S) for _ in range(5)]
    st = _hip.stream()
    _hip.call("mx_rate_track_nodes", m.data_ptr(), stride, B, n, float(sr), _hip.ptr(starts), S, W, *grid, *buffers, st)
    _hip.call("mx_rate_track_path", B, n, float(sr), _hip.ptr(starts), S, W, *grid, D, rw, pw, *buffers, _hip.ptr(shape),
              _hip.ptr(grid_k), _hip.ptr(grid_j), _hip.ptr(cost), _hip.ptr(per_shape), st)
    _hip.call("mx_rate_track_refine", m.data_ptr(), stride, B, n, float(sr), _hip.ptr(starts), S, W, *grid, L, _hip.ptr(shape),
              _hip.ptr(grid_k), _hip.ptr(grid_j), *[_hip.ptr(o) for o in fitted], buffers[2], buffers[3], st)
    return RateTrack(shape, grid_k, grid_j, *fitted, cost, per_shape, starts, W, n, float(sr))


def synth_from_rate_track(rt: RateTrack, row: int = 0) -> T:
    """(n_points,) fp32: the S slice templates of row ``row`` (``modulations.synth_from_fit``, one batched ``mx_lfo_synth`` of S
    rows at the track's point rate ``rt.sr``) joined by ``file_eval.stitch_lfo`` with n_f = N = ``slice_points`` and
    n_t = L = ``n_points``: K22's positions are then integers, its interpolation is exact and what remains is its sin^2 taper.
    Piecewise: the join is a cross-fade of neighbouring templates, not a phase-continuous oscillator."""
    from .file_eval import stitch_lfo
    S = rt.starts.numel()
    fit = LFOFit(rt.shape[row].expand(S).contiguous(), rt.rate_hz[row], rt.phase[row], rt.amp[row], rt.offset[row], rt.resid[row])
    templates = synth_from_fit(fit, rt.slice_points, rt.sr)
    return stitch_lfo(templates, rt.starts, L=rt.n_points, N=rt.slice_points, n_t=rt.n_points)[0]


def rate_at(rt: RateTrack, sr: Optional[float] = None) -> Tuple[T, T]:
    """(times_s (S,) fp64, rate_hz (B, S)): the slice centres in seconds -- point i of a row sits at i / sr, ``sr`` defaulting
    to the fit's -- and the refined rates there.  The contour is piecewise constant: one rate a slice."""
    times = (rt.starts.to(torch.float64) + 0.5 * (rt.slice_points - 1)) / float(rt.sr if sr is None else sr)
    return times, rt.rate_hz

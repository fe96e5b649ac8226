"""Host mirror of mod_extraction/modulations.py on HIP tensors.

``make_mod_signal`` keeps the reference signature (modulations.py:16-21) and runs the ``mx_lfo_synth``
kernel; ``make_mod_signals`` is the batched form the training loop uses (one launch for the whole
batch, optional crop offset and on-the-fly resampling).
"""
import ctypes
import math
from typing import List, NamedTuple, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor as T

from . import _hip

SHAPE_IDS = {"cos": 0, "rect_cos": 1, "inv_rect_cos": 2, "tri": 3, "saw": 4, "rsaw": 5, "sqr": 6}


def _device(device=None) -> torch.device:
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def make_mod_signals(n_samples: int, sr: float, freq: T, phase: T, shape: Optional[T] = None,
                     exp: Optional[T] = None, start: Optional[T] = None,
                     n_out: Optional[int] = None, out: Optional[T] = None) -> T:
    """Batched LFO synthesis: freq/phase/exp (B,) fp32, shape/start (B,) int32, all on the device.
    Returns (B, n_out or n_samples)."""
    B = freq.numel()
    n_out = n_samples if n_out is None else n_out
    y = out if out is not None else torch.empty((B, n_out), device=freq.device, dtype=torch.float32)
    _hip.call("mx_lfo_synth", _hip.ptr(freq), _hip.ptr(phase), _hip.ptr(shape), _hip.ptr(exp),
              _hip.ptr(start), B, n_samples, n_out, float(sr), _hip.ptr(y), _hip.stream())
    return y


def make_mod_signal(n_samples: int, sr: float, freq: float, phase: float = 0.0, shape: str = "cos",
                    exp: float = 1.0, device=None) -> T:
    assert n_samples > 0
    assert 0.0 < freq < sr / 2.0
    assert -2 * math.pi <= phase <= 2 * math.pi
    assert shape in SHAPE_IDS
    assert exp > 0
    dev = _device(device)
    f = torch.tensor([float(freq)], device=dev, dtype=torch.float32)
    p = torch.tensor([float(phase)], device=dev, dtype=torch.float32)
    s = torch.tensor([SHAPE_IDS[shape]], device=dev, dtype=torch.int32)
    e = torch.tensor([float(exp)], device=dev, dtype=torch.float32)
    return make_mod_signals(n_samples, sr, f, p, s, e).view(-1)


# ---- K9: corner bookkeeping (modulations.py:219-363), bit-exact on the device ------------------
def _rows2d(x: T):
    assert x.ndim == 2
    return x.contiguous().float()


def smoothen(x: T, smooth_n_frames: int) -> T:
    """modulations.py:359-363."""
    if smooth_n_frames <= 1:
        return x
    lead = x.shape[:-1]
    xc = x.reshape(-1, x.size(-1)).contiguous().float()
    n_out = xc.size(-1) - smooth_n_frames + 1
    out = torch.empty((xc.size(0), n_out), device=xc.device, dtype=torch.float32)
    _hip.call("mx_smoothen", _hip.ptr(xc), xc.size(0), xc.size(-1), smooth_n_frames, _hip.ptr(out), _hip.stream())
    return out.view(lead + (n_out,))


def find_corners(mod_sig: T) -> (T, T):
    """modulations.py:219-238: float 0/1 maps of top and bottom corners."""
    m = _rows2d(mod_sig)
    top, bot = torch.empty_like(m), torch.empty_like(m)
    _hip.call("mx_find_corners", _hip.ptr(m), m.size(0), m.size(1), _hip.ptr(top), _hip.ptr(bot), _hip.stream())
    return top, bot


def stretch_corners(mod_sig: T, max_n_corners: int = 10, smooth_n_frames: int = 32) -> T:
    """modulations.py:294-307."""
    m = _rows2d(smoothen(mod_sig, smooth_n_frames))
    out = torch.empty_like(m)
    _hip.call("mx_stretch_corners", _hip.ptr(m), m.size(0), m.size(1), int(max_n_corners), _hip.ptr(out),
              _hip.stream())
    return out


class _SmoothenFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: T, k: int):
        ctx.k = k
        return smoothen(x.detach(), k)

    @staticmethod
    def backward(ctx, dy: T):
        return smoothen_bwd(dy.contiguous(), ctx.k), None


def smoothen_with_grad(x: T, smooth_n_frames: int) -> T:
    """``smoothen`` as an autograd node (forward ``mx_smoothen``, backward its transpose): lightning.py:117-119 while training."""
    return x if smooth_n_frames <= 1 else _SmoothenFn.apply(x, smooth_n_frames)


def smoothen_bwd(dy: T, smooth_n_frames: int) -> T:
    """Transpose of ``smoothen``: the same moving average over the zero-padded gradient."""
    if smooth_n_frames <= 1:
        return dy
    k = smooth_n_frames
    return smoothen(torch.nn.functional.pad(dy, (k - 1, k - 1)), k)


def stretch_corners_bwd(mod_sig: T, d_out: T, max_n_corners: int = 10, smooth_n_frames: int = 32) -> T:
    """Gradient of ``stretch_corners(mod_sig, ...)`` w.r.t. ``mod_sig`` given the gradient w.r.t. its result (the reference's
    _stretch_corners is differentiable torch code, modulations.py:260-291; corner positions carry no gradient)."""
    m = _rows2d(smoothen(mod_sig, smooth_n_frames))
    g = _rows2d(d_out)
    assert g.shape == m.shape
    dm = torch.empty_like(m)
    _hip.call("mx_stretch_corners_bwd", _hip.ptr(m), _hip.ptr(g), m.size(0), m.size(1), int(max_n_corners), _hip.ptr(dm),
              _hip.stream())
    return smoothen_bwd(dm, smooth_n_frames)


def valid_mod_sig_mask(mod_sig: T, min_top_corners: int = 1, max_top_corners: int = 6,
                       min_bottom_corners: int = 1, max_bottom_corners: int = 6,
                       min_fraction_between_corners: float = 0.10) -> T:
    """check_mod_sig (modulations.py:311-343) for every row: (B,) int32 0/1 on the device."""
    m = _rows2d(mod_sig)
    valid = torch.empty(m.size(0), device=m.device, dtype=torch.int32)
    _hip.call("mx_check_mod_sig", _hip.ptr(m), m.size(0), m.size(1), min_top_corners, max_top_corners,
              min_bottom_corners, max_bottom_corners, int(min_fraction_between_corners * m.size(1)),
              _hip.ptr(valid), _hip.stream())
    return valid


def mod_sig_to_corners(mod_sig: T, n_frames: int) -> (T, T):
    """modulations.py:212-216: corners of the LFOs resampled to ``n_frames`` points."""
    from . import util
    assert mod_sig.ndim == 2
    return find_corners(util.linear_interpolate_last_dim(mod_sig, n_frames))


def check_mod_sig(mod_sig: T, top_corners: T, bottom_corners: T, min_top_corners: int = 1, max_top_corners: int = 6,
                  min_bottom_corners: int = 1, max_bottom_corners: int = 6,
                  min_fraction_between_corners: float = 0.10) -> bool:
    """modulations.py:311-343 for ONE LFO and the corner maps the caller holds (the batched form on the device is
    ``valid_mod_sig_mask``): corner counts within bounds and neighbouring corners of a kind at least
    ``int(min_fraction_between_corners * n)`` frames apart."""
    assert mod_sig.ndim == 1 and mod_sig.shape == top_corners.shape == bottom_corners.shape
    min_gap = int(min_fraction_between_corners * mod_sig.size(0))
    for corners, lo, hi in ((top_corners, min_top_corners, max_top_corners),
                            (bottom_corners, min_bottom_corners, max_bottom_corners)):
        if not lo <= int(corners.sum()) <= hi:
            return False
    for corners in (top_corners, bottom_corners):
        at = torch.nonzero(corners == 1).view(-1)
        if at.numel() > 1 and int((at[1:] - at[:-1]).min()) < min_gap:
            return False
    return True


def corners_to_mod_sig(top_corners: T, bottom_corners: T) -> T:
    """modulations.py:241-257: the triangle LFO through the corners of ONE row -- 1 at the top corners, 0 at the bottom
    ones, straight lines in between, 0 outside the first / last corner and when either kind is absent."""
    assert top_corners.ndim == 1 and top_corners.shape == bottom_corners.shape
    out = torch.zeros(top_corners.shape, dtype=torch.float32, device=top_corners.device)
    if float(top_corners.max()) == 0 or float(bottom_corners.max()) == 0:
        return out
    knots = sorted([(int(i), 1.0) for i in torch.nonzero(top_corners == 1).view(-1)]
                   + [(int(i), 0.0) for i in torch.nonzero(bottom_corners == 1).view(-1)])
    for (l, lv), (r, rv) in zip(knots[:-1], knots[1:]):
        out[l:r + 1] = torch.linspace(lv, rv, r - l + 1, device=out.device)
    return out


def find_valid_mod_sig_indices(mod_sig: T) -> List[int]:
    """modulations.py:346-356 (host list, like the reference; one small D2H copy)."""
    return torch.nonzero(valid_mod_sig_mask(mod_sig)).view(-1).tolist()


def make_rand_mod_signal(batch_size: int, n_samples: int, sr: float, freq_min: float, freq_max: float,
                         shapes_gt: Optional[Sequence[str]] = None, shapes: Optional[List[str]] = None,
                         phase_gt: Optional[T] = None, phase_error: float = 0.5,
                         freq_gt: Optional[T] = None, freq_error: float = 0.25, device=None) -> T:
    """modulations.py:60-101: the per-item host RNG draws are kept in the reference's order; the
    batch of LFOs is then synthesised by one ``mx_lfo_synth`` launch."""
    from . import util
    if shapes is None:
        shapes = ["cos", "tri", "rect_cos", "inv_rect_cos", "saw", "rsaw"]
    freqs, phases, shape_ids = [], [], []
    # ground-truth rows are perturbed with the reference's own fp32 tensor arithmetic (0-dim CPU tensors, in-place
    # add / multiply, then the wrap / clip), on private copies: the reference mutates the caller's fx_params here
    phase_gt = None if phase_gt is None else phase_gt.detach().to("cpu", torch.float32).clone()
    freq_gt = None if freq_gt is None else freq_gt.detach().to("cpu", torch.float32).clone()
    for idx in range(batch_size):
        if phase_gt is not None:
            assert phase_gt.size(0) == batch_size
            phase = phase_gt[idx]
            if phase_error > 0:
                phase += util.sample_uniform(-1.0, 1.0) * math.pi * phase_error
                phase = (phase + (2 * math.pi)) % (2 * math.pi)
        else:
            phase = util.sample_uniform(0.0, 2 * math.pi)
        if freq_gt is not None:
            assert freq_gt.size(0) == batch_size
            freq = freq_gt[idx]
            if freq_error > 0:
                freq *= util.sample_uniform(1.0 - freq_error, 1.0 + freq_error)
                freq = torch.clip(freq, freq_min, freq_max)
        else:
            freq = util.sample_uniform(freq_min, freq_max)
        shape = shapes_gt[idx] if shapes_gt is not None else util.choice(shapes)
        freqs.append(float(freq)); phases.append(float(phase)); shape_ids.append(SHAPE_IDS[shape])
    dev = _device(device)
    return make_mod_signals(n_samples, sr, torch.tensor(freqs, dtype=torch.float32, device=dev),
                            torch.tensor(phases, dtype=torch.float32, device=dev),
                            torch.tensor(shape_ids, dtype=torch.int32, device=dev))


# ---- evaluation LFO variants (modulations.py:104-210) ------------------------------------------
# Per-item data-generation helpers of the eval configs (eval_lfo_quasi / combined / distorted): host
# control flow and host RNG draws in the reference's order; every array operation (LFO synthesis,
# corner detection, resampling) runs in the device kernels above.
def _time_stretch_section(section: T, l_min: float, l_max: float, r_min: float, r_max: float,
                          lr_split: float = 0.5) -> T:
    from . import util
    size = section.size(0)
    if util.sample_uniform(0.0, 1.0) < lr_split:
        x = int((util.sample_uniform(l_min, l_max) * size) + 0.5)
        new_size = max(2, size - x)
    else:
        x = int((util.sample_uniform(r_min, r_max) * size) + 0.5)
        new_size = size + x
    return util.linear_interpolate_last_dim(section.contiguous(), new_size, align_corners=True)


def _corner_indices(corners: T) -> List[int]:
    return [int(c) for c in (corners.view(-1) == 1).nonzero(as_tuple=True)[0].tolist()]


def make_quasi_periodic(mod_sig: T, l_min: float = 0.2, l_max: float = 0.2, r_min: float = 0.2,
                        r_max: float = 0.2, lr_split: float = 0.5) -> T:
    """modulations.py:121-160: time-stretch every corner-to-corner section by a random amount."""
    from . import util
    assert mod_sig.ndim == 1
    top, bot = find_corners(mod_sig.unsqueeze(0))
    corners = top if float(top.sum()) > float(bot.sum()) else bot
    idx = _corner_indices(corners)
    if len(idx) < 2:
        return mod_sig
    sections, total, prev = [], 0, 0
    for c in idx:
        new_section = _time_stretch_section(mod_sig[prev:c + 1], l_min, l_max, r_min, r_max, lr_split)[:-1]
        total += new_section.size(0)
        sections.append(new_section)
        prev = c
    n = mod_sig.size(0)
    tail = mod_sig[prev:n]
    total += tail.size(0)
    if total < n:
        tail = util.linear_interpolate_last_dim(tail.contiguous(), tail.size(0) + (n - total), align_corners=True)
    sections.append(tail)
    return torch.cat(sections, dim=0)[:n]


def make_combined_mod_sig(n_samples: int, sr: float, freq: float, phase: float, shapes: List[str],
                          device=None) -> T:
    """modulations.py:191-210: a new random shape between every pair of bottom corners."""
    from . import util
    mod_sig = make_mod_signal(n_samples, sr, freq, phase, shape=util.choice(shapes), device=device)
    _, bot = find_corners(mod_sig.unsqueeze(0))
    idx = _corner_indices(bot)
    for a, b in zip(idx[:-1], idx[1:]):
        n = b - a + 1
        mod_sig[a:b + 1] = make_mod_signal(n, n, freq=1.0, phase=0.0, shape=util.choice(shapes), device=mod_sig.device)
    return mod_sig


def make_concave_convex_mod_sig(n_samples: int, sr: float, freq: float, phase: float = 0.0,
                                concave_min: float = 0.2, concave_max: float = 1.0, convex_min: float = 1.0,
                                convex_max: float = 3.0, concave_prob: float = 0.5, device=None) -> T:
    """modulations.py:163-188: triangle LFO with a random exponent per monotone segment."""
    from . import util
    mod_sig = make_mod_signal(n_samples, sr, freq, phase, shape="tri", device=device)
    top, bot = find_corners(mod_sig.unsqueeze(0))
    idx = _corner_indices(top + bot) + [mod_sig.size(0)]
    exp = torch.ones_like(mod_sig)
    prev = 0
    for c in idx:
        if util.sample_uniform(0.0, 1.0) < concave_prob:
            v = util.sample_uniform(concave_min, concave_max)
        else:
            v = util.sample_uniform(convex_min, convex_max)
        exp[prev:c] = v
        prev = c
    return mod_sig ** exp


# ---- the same variants for a whole batch (csrc/lfo_variants.hip) --------------------------------
# The per-item functions above draw a data-dependent number of host random values per LFO and pull the corner indices to
# the host; the batch forms take the draws as FIXED-WIDTH tables (S entries per row) that the kernel consumes in corner
# order: one launch per batch, nothing returns to the host.  With the tables filled in the per-item order they compute the
# per-item functions' outputs bit for bit (tests/test_gpu_lfo_variants.py).
def draw_quasi_tables(B: int, S: int, l_min: float = 0.2, l_max: float = 0.2, r_min: float = 0.2, r_max: float = 0.2,
                      lr_split: float = 0.5) -> (T, T):
    """Host draws of ``_time_stretch_section`` for B rows of up to S sections: two ``torch.rand(B, S)`` (split, amount).
    Returns ``shrink`` (B, S) int32 (1 = the section shrinks) and ``amount`` (B, S) float32, in [l_min, l_max] where
    ``shrink`` is set and in [r_min, r_max] elsewhere (``util.sample_uniform``'s own fp32 expression)."""
    u_split, u_amt = torch.rand(B, S), torch.rand(B, S)
    shrink = u_split.double() < lr_split
    amount = torch.where(shrink, u_amt * (l_max - l_min) + l_min, u_amt * (r_max - r_min) + r_min)
    return shrink.to(torch.int32), amount.to(torch.float32)


def draw_combined_table(B: int, S: int, shapes: Union[int, Sequence[str]]) -> T:
    """Host draws of ``make_combined_mod_sig`` for B rows of up to S corner pairs: ``torch.randint(0, n_shapes, (B, S + 1))``
    (column 0: the base shape), mapped to ``SHAPE_IDS`` when ``shapes`` is the list of names the indices choose from
    (an int ``n_shapes`` chooses among the first ``n_shapes`` ids).  Returns (B, S + 1) int32."""
    n_shapes = shapes if isinstance(shapes, int) else len(shapes)
    idx = torch.randint(0, n_shapes, (B, S + 1))
    if not isinstance(shapes, int):
        idx = torch.tensor([SHAPE_IDS[s] for s in shapes], dtype=torch.int64)[idx]
    return idx.to(torch.int32)


def make_quasi_periodic_batch(mod_sig: T, shrink: T, amount: T, out: Optional[T] = None) -> (T, T):
    """``make_quasi_periodic`` on every row of ``mod_sig`` (B, n) in one ``mx_lfo_quasi_periodic`` launch: section s of row b
    shrinks (``shrink[b, s]`` != 0) or grows by ``int(amount[b, s] * size + 0.5)`` points.  Rows with fewer than 2 or more
    than S = ``shrink.size(1)`` corners come back unchanged.  Returns ``(out, n_corners)``, both on the device;
    ``n_corners`` (B,) int32 is the real corner count of every row."""
    m = _rows2d(mod_sig)
    assert shrink.ndim == 2 and shrink.shape == amount.shape and shrink.size(0) == m.size(0)
    sh = shrink.to(torch.int32).contiguous()
    am = amount.to(torch.float32).contiguous()
    if out is None:
        out = torch.empty_like(m)
    assert out.shape == m.shape and out.dtype == torch.float32 and out.data_ptr() != m.data_ptr()
    n_corners = torch.empty(m.size(0), device=m.device, dtype=torch.int32)
    _hip.call("mx_lfo_quasi_periodic", _hip.ptr(m), _hip.ptr(sh), _hip.ptr(am), m.size(0), m.size(1), sh.size(1),
              _hip.ptr(out), _hip.ptr(n_corners), _hip.stream())
    return out, n_corners


def make_combined_mod_sigs(n_samples: int, sr: float, freq: T, phase: T, shape_table: T) -> (T, T):
    """``make_combined_mod_sig`` for a batch in one ``mx_lfo_combined`` launch: freq / phase (B,) fp32 on the device,
    ``shape_table`` (B, S + 1) int32 shape ids -- column 0 the base shape, column s + 1 the shape between bottom corners s
    and s + 1 (pairs beyond S keep the base).  Returns ``(out (B, n_samples), n_corners (B,) int32)``."""
    B = freq.numel()
    assert shape_table.ndim == 2 and shape_table.size(0) == B and shape_table.size(1) >= 2
    tab = shape_table.to(torch.int32).contiguous()
    out = torch.empty((B, n_samples), device=freq.device, dtype=torch.float32)
    n_corners = torch.empty(B, device=freq.device, dtype=torch.int32)
    _hip.call("mx_lfo_combined", _hip.ptr(freq), _hip.ptr(phase), _hip.ptr(tab), B, n_samples, tab.size(1) - 1, float(sr),
              _hip.ptr(out), _hip.ptr(n_corners), _hip.stream())
    return out, n_corners


# ---- K18: the inverse of ``make_mod_signals`` (csrc/lfo_fit.hip) ---------------------------------
LFO_SHAPES = ("cos", "rect_cos", "inv_rect_cos", "tri", "saw", "rsaw")       # the default set of the fit: all but "sqr"
SHAPE_NAMES = tuple(sorted(SHAPE_IDS, key=SHAPE_IDS.get))


class LFOFit(NamedTuple):
    """What ``fit_lfo`` returns: (B,) device tensors, ``shape`` int32 (ids of ``SHAPE_IDS``), the rest fp32;
    ``per_shape_resid`` (B, 7) fp32 (+inf where a shape was not allowed) or None.  ``offset + amp * make_mod_signals(n, sr,
    rate_hz, phase, shape)`` is the fitted template (``synth_from_fit``); ``resid`` is its squared error over the row's
    centred energy."""
    shape: T
    rate_hz: T
    phase: T
    amp: T
    offset: T
    resid: T
    per_shape_resid: Optional[T] = None

    def shape_names(self) -> List[str]:
        """The fitted shapes by name (copies ``shape`` to the host: a sync)."""
        return [SHAPE_NAMES[i] for i in self.shape.tolist()]


def fit_shape_mask(shapes: Sequence[str]) -> int:
    """Bit mask over ``SHAPE_IDS`` of a non-empty list of shape names (ValueError otherwise)."""
    if isinstance(shapes, str) or len(shapes) == 0:
        raise ValueError(f"fit_lfo: shapes must be a non-empty list of names from {list(SHAPE_IDS)}, got {shapes!r}")
    mask = 0
    for s in shapes:
        if s not in SHAPE_IDS:
            raise ValueError(f"fit_lfo: unknown LFO shape {s!r} (known: {list(SHAPE_IDS)})")
        mask |= 1 << SHAPE_IDS[s]
    return mask


def fit_rate_window(rate_hz, sr: float) -> Tuple[float, float]:
    """(f_min, f_max) of a two-element rate window with 0 < f_min <= f_max < sr / 2 (ValueError otherwise)."""
    try:
        f_min, f_max = (float(v) for v in rate_hz)
    except (TypeError, ValueError):
        raise ValueError(f"fit_lfo: rate_hz must be a (min, max) pair in Hz, got {rate_hz!r}") from None
    if not (sr > 0.0 and 0.0 < f_min <= f_max < sr / 2.0):
        raise ValueError(f"fit_lfo: need 0 < rate_hz[0] <= rate_hz[1] < sr / 2, got {rate_hz!r} at sr = {sr}")
    return f_min, f_max


FIT_MIN_POINTS = 16                             # FIT_MIN_N of csrc/lfo_fit_common.h
FIT_MAX_POINTS = 4096                           # FIT_MAX_N of csrc/lfo_fit.hip: the longest row mx_lfo_fit takes
FIT_MAX_RATES = 512                             # FIT_MAX_K there: the most rates of its grid
TRACK_FIT_MAX_POINTS = 1 << 20                  # MX_TRACK_FIT_MAX_N of csrc/track_fit_abi.h
TRACK_FIT_MAX_RATES = 1 << 20                   # MX_TRACK_FIT_MAX_K there
TRACK_FIT_ROW_TILE = _hip.TRACK_FIT_ROW_TILE    # MX_TRACK_FIT_ROW_TILE there: the points of a row mx_track_fit stages at a time


def _fl32(v: float) -> float:
    """``v`` rounded to fp32, as a float: what the C ABI receives for a ``float`` parameter."""
    return ctypes.c_float(v).value


def fit_plan(n: int, sr: float, rate_hz=(0.25, 8.0), rate_div: int = 4) -> Tuple[str, int]:
    """(route, K) of a fit of n-point rows: ``"lfo_fit"`` (K18, one workgroup a row: n <= 4096 and K <= 512) or
    ``"track_fit"`` (K23, a grid of candidate tiles: n <= 2^20, K <= 2^20), and the number of rates
    K = floor((f_max - f_min) / df) + 1, df = 1 / (rate_div (n / sr)): fp64 on the fp32 roundings of the window and of sr,
    the formula of both libraries' entry points.  Pure host arithmetic.  A row below 16 points, or a ``rate_div`` outside
    1 .. 16, has no grid: up to 4096 points it goes to ``mx_lfo_fit`` with K = 0, which refuses it as it always has; a longer
    one is a ValueError, as are n > 2^20 and K > 2^20."""
    f_min, f_max = fit_rate_window(rate_hz, float(sr))
    n, rate_div = int(n), int(rate_div)
    if n > TRACK_FIT_MAX_POINTS:
        raise ValueError(f"fit_lfo: rows of {n} points; the fit takes at most {TRACK_FIT_MAX_POINTS}")
    if n < FIT_MIN_POINTS or not 1 <= rate_div <= 16:
        if n <= FIT_MAX_POINTS:
            return "lfo_fit", 0
        raise ValueError(f"fit_lfo: rate_div must be in 1 .. 16, got {rate_div}")
    df = 1.0 / (rate_div * (n / _fl32(float(sr))))
    K = int(math.floor((_fl32(f_max) - _fl32(f_min)) / df)) + 1
    if n <= FIT_MAX_POINTS and K <= FIT_MAX_RATES:
        return "lfo_fit", K
    if K > TRACK_FIT_MAX_RATES:
        raise ValueError(f"fit_lfo: the rate window {rate_hz!r} needs {K} rates on {n} points at rate_div = {rate_div}; the "
                         f"fit takes at most {TRACK_FIT_MAX_RATES}")
    return "track_fit", K


def fit_lfo(mod_sig: T, sr: float, rate_hz=(0.25, 8.0), shapes: Sequence[str] = LFO_SHAPES, rate_div: int = 4,
            n_phases: int = 32, n_rounds: int = 4, per_shape: bool = False) -> LFOFit:
    """Rate, phase and shape of every row of ``mod_sig`` ((B, n) or (n,), fp32, on the device; ``sr`` the rate of its
    points, 172.5 for 345 points of a 2 s clip): a grid search over the rate window ``rate_hz`` (spacing ``sr / (rate_div n)``)
    and ``n_phases`` centre phases, ``n_rounds`` rounds of 5 x 5 refinement, per allowed shape, with a non-negative amplitude
    and a free offset (include/modex_hip.h, K18, has the definition).  Rows a row stride apart (inner stride 1) are read in
    place.  ``fit_plan`` picks the route: rows of at most 4096 points on a grid of at most 512 rates are one ``mx_lfo_fit``
    launch; longer rows or finer grids (to 2^20 points, 2^20 rates) go to ``mx_track_fit`` (K23, csrc/track_fit_abi.h), the
    same function on a grid of workgroups, with a workspace from ``torch.empty``."""
    mask = fit_shape_mask(shapes)
    f_min, f_max = fit_rate_window(rate_hz, float(sr))
    if not isinstance(mod_sig, torch.Tensor) or mod_sig.ndim not in (1, 2) or mod_sig.dtype != torch.float32:
        raise ValueError("fit_lfo: mod_sig must be an fp32 tensor of shape (B, n) or (n,)")
    if not mod_sig.is_cuda:
        raise ValueError("fit_lfo: mod_sig must be on a HIP device (there is no CPU fallback)")
    m = mod_sig.detach()
    m = m.unsqueeze(0) if m.ndim == 1 else m
    B, n = m.shape
    if B == 0:
        raise ValueError("fit_lfo: mod_sig has no rows")
    route, _ = fit_plan(n, sr, (f_min, f_max), rate_div)
    if route == "track_fit" and not (4 <= int(n_phases) <= 128 and 0 <= int(n_rounds) <= 8):
        raise ValueError(f"fit_lfo: need 4 <= n_phases <= 128 and 0 <= n_rounds <= 8, got {n_phases!r} and {n_rounds!r}")
    if m.stride(1) != 1 or (B > 1 and m.stride(0) < n):
        m = m.contiguous()
    stride = max(m.stride(0), n) if B > 1 else n
    dev = m.device
    grid = (float(sr), f_min, f_max, mask, int(rate_div), int(n_phases), int(n_rounds))
    ws_args = ()
    if route == "track_fit":
        sizes = (ctypes.c_int64 * 2)()                                  # K and the workspace's bytes, from the library
        _hip.call("mx_track_fit_plan", B, n, *grid, ctypes.addressof(sizes), ctypes.addressof(sizes) + 8)
        ws = torch.empty((sizes[1] + 7) // 8, device=dev, dtype=torch.float64)
        ws_args = (ws.data_ptr(), ws.numel() * 8)
    out = [torch.empty(B, device=dev, dtype=torch.int32)] + [torch.empty(B, device=dev, dtype=torch.float32) for _ in range(5)]
    table = torch.empty((B, 7), device=dev, dtype=torch.float32) if per_shape else None
    _hip.call("mx_lfo_fit" if route == "lfo_fit" else "mx_track_fit", m.data_ptr(), stride, B, n, *grid,
              *[_hip.ptr(o) for o in out], _hip.ptr(table), *ws_args, _hip.stream())
    return LFOFit(*out, table)


def synth_from_fit(fit: LFOFit, n_samples: int, sr: float, start: Union[None, int, T] = None,
                   n_out: Optional[int] = None) -> T:
    """``offset + amp * make_mod_signals(n_samples, sr, rate_hz, phase, shape, start=start, n_out=n_out)``: (B, n_out or
    n_samples).  With the ``n_samples`` and ``sr`` of the fitted rows this is the fitted template; ``start`` (an int, or a
    (B,) int32 tensor) continues it beyond the clip: ``start = n`` gives the next ``n_samples`` points."""
    if isinstance(start, int):
        start = torch.full_like(fit.shape, start)
    sig = make_mod_signals(n_samples, sr, fit.rate_hz, fit.phase, fit.shape, start=start, n_out=n_out)
    return fit.offset.unsqueeze(1) + fit.amp.unsqueeze(1) * sig

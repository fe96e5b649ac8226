"""A whole recording: the extractor's LFO along the file, the re-render from it, and how close that is -- no counterpart in
the reference.

    window_starts      where the model's N-sample windows sit on a file of L samples
    stitch_lfo         K22 (csrc/lfo_stitch.hip; include/modex_hip.h has the definition): the windows' LFOs -> one track
    extract_lfo_track  the model over every window of a file, stitched
    render_file        ``LFOExtractionThroughEffect.render`` on the file as ONE row: the delay line starts where the recording
                       does, so there is no warm-up to mask ("Warm-up of a chunk cut from a file")
    score_pair         lag / polarity, track, ``modulations.fit_lfo`` on the track, re-render, ONE gain or FIR per file, and
                       the step's audio losses on the matched render

Device tensors throughout; nothing here synchronises with the host (``window_starts`` is host arithmetic on Python ints).
"""
from typing import Dict, List, NamedTuple, Optional, Sequence, Union

import torch
from torch import Tensor as T

from . import _hip
from .modulations import FIT_MAX_POINTS, FIT_MAX_RATES     # K18's limits: fit_track keeps its launch inside them

MAX_WINDOWS = 1 << 20                           # MX_STITCH_MAX_WINDOWS


class LfoTrack(NamedTuple):
    """What ``extract_lfo_track`` returns: ``track`` (n_t,) fp32, ``cover`` (n_t,) int32 (windows per point), ``windows``
    (W, n_f) fp32 (the model's LFO of every window) and ``starts`` (the W first samples, a list of ints)."""
    track: T
    cover: T
    windows: T
    starts: List[int]


def _int(v, name: str, fn: str) -> int:
    if isinstance(v, bool) or not isinstance(v, int):
        raise ValueError(f"{fn}: {name} must be an int, got {v!r}")
    return v


def window_starts(L: int, N: int, hop: Optional[int] = None) -> List[int]:
    """The first samples of the N-sample windows on a file of L samples: 0, hop, 2 hop, ... while the window fits, and one
    last window right-aligned at L - N if those leave the end uncovered.  ``hop`` defaults to N // 2; 1 <= hop <= N, so
    every sample is covered.  L < N is a ValueError (the model is not shown a padded window)."""
    fn = "window_starts"
    L, N = _int(L, "L", fn), _int(N, "N", fn)
    if N < 1:
        raise ValueError(f"{fn}: N must be at least 1, got {N}")
    if L < N:
        raise ValueError(f"{fn}: a file of L = {L} samples is shorter than one window of N = {N}")
    hop = max(1, N // 2) if hop is None else _int(hop, "hop", fn)
    if not 1 <= hop <= N:
        raise ValueError(f"{fn}: hop must be in 1 .. N = {N}, got {hop}")
    starts = list(range(0, L - N + 1, hop))
    if starts[-1] != L - N:
        starts.append(L - N)
    return starts


def default_track_points(L: int, N: int, n_f: int) -> int:
    """max(2, round(L n_f / N)): the windows' own point rate carried over the file."""
    return max(2, int(round(L * n_f / N)))


def stitch_lfo(lfo_windows: T, starts: Union[Sequence[int], T], L: int, N: int, n_t: Optional[int] = None,
               out: Optional[T] = None):
    """(track (n_t,) fp32, cover (n_t,) int32) from ``lfo_windows`` (W, n_f) fp32 on the device, window w covering the samples
    ``starts[w] .. starts[w] + N - 1`` of a file of L samples, in one ``mx_lfo_stitch`` launch: every track point is the
    sin^2-tapered mean of the windows that cover it, each interpolated linearly at the point (include/modex_hip.h, K22).
    ``starts``: ascending ints, or an int64 device tensor.  ``n_t`` defaults to ``default_track_points``.  ``out``: an fp32
    (n_t,) device tensor with unit stride that receives the track."""
    fn = "stitch_lfo"
    if not isinstance(lfo_windows, torch.Tensor) or lfo_windows.dtype != torch.float32 or lfo_windows.ndim != 2:
        raise ValueError(f"{fn}: lfo_windows must be an fp32 tensor of shape (W, n_f)")
    if not lfo_windows.is_cuda:
        raise ValueError(f"{fn}: lfo_windows must be on a HIP device (there is no CPU fallback)")
    W, n_f = lfo_windows.shape
    L, N = _int(L, "L", fn), _int(N, "N", fn)
    if W < 1 or n_f < 2:
        raise ValueError(f"{fn}: need at least one window of at least two points, got {tuple(lfo_windows.shape)}")
    if N < 2 or L < N:
        raise ValueError(f"{fn}: need 2 <= N <= L, got N = {N}, L = {L}")
    n_t = default_track_points(L, N, n_f) if n_t is None else _int(n_t, "n_t", fn)
    if n_t < 2:
        raise ValueError(f"{fn}: n_t must be at least 2, got {n_t}")
    dev = lfo_windows.device
    if isinstance(starts, torch.Tensor):
        if starts.dtype != torch.int64 or starts.shape != (W,) or starts.device != dev:
            raise ValueError(f"{fn}: starts must be an int64 tensor of shape ({W},) on the windows' device")
        st = starts.contiguous()
    else:
        starts = [_int(s, "a start", fn) for s in starts]
        if len(starts) != W:
            raise ValueError(f"{fn}: {len(starts)} starts for {W} windows")
        if any(b < a for a, b in zip(starts, starts[1:])) or starts[0] < 0 or starts[-1] > L - N:
            raise ValueError(f"{fn}: starts must ascend inside 0 .. L - N = {L - N}")
        st = torch.tensor(starts, dtype=torch.int64, device=dev)
    if out is None:
        out = torch.empty(n_t, device=dev, dtype=torch.float32)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.shape != (n_t,) or out.device != dev
          or out.stride(0) != 1):
        raise ValueError(f"{fn}: out must be an fp32 tensor of shape ({n_t},) with unit stride on the windows' device")
    cover = torch.empty(n_t, device=dev, dtype=torch.int32)
    _hip.call("mx_lfo_stitch", _hip.ptr(lfo_windows.detach().contiguous()), _hip.ptr(st), W, n_f, N, L, n_t, out.data_ptr(),
              _hip.ptr(cover), _hip.stream())
    return out, cover


def _file_row(x, name: str, fn: str) -> T:
    """(L,) view of an fp32 device tensor of shape (L,) or (1, L)."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not (x.ndim == 1 or (x.ndim == 2 and x.size(0) == 1)):
        raise ValueError(f"{fn}: {name} must be an fp32 tensor of shape (L,) or (1, L)")
    if not x.is_cuda:
        raise ValueError(f"{fn}: {name} must be on a HIP device (there is no CPU fallback)")
    x = x.detach().reshape(-1)
    return x if x.stride(0) == 1 else x.contiguous()


def _windows_of(x: T, starts: List[int], i: int, j: int, N: int, hop: int) -> T:
    """(j - i, 1, N): windows i .. j - 1 of the file row ``x``, stacked from views (the regular ones one ``unfold``, a
    right-aligned last one an ``as_strided``)."""
    regular = (x.numel() - N) // hop + 1                            # the rest, if any, is the right-aligned last window
    parts = []
    if i < min(j, regular):
        parts.append(x.unfold(0, N, hop)[i:min(j, regular)])
    if j > regular:
        parts.append(torch.as_strided(x, (1, N), (N, 1), x.storage_offset() + starts[-1]))
    return (parts[0] if len(parts) == 1 else torch.cat(parts, 0)).unsqueeze(1).contiguous()


def extract_lfo_track(model, wet: T, dry: Optional[T] = None, n_samples: int = 88200, hop: Optional[int] = None,
                      batch_size: int = 32) -> LfoTrack:
    """The extractor's LFO along a whole recording.  ``wet`` (and ``dry``, for a model that is shown both) are (L,) or (1, L)
    fp32 on the device; the model sees every window of ``window_starts(L, n_samples, hop)``, ``batch_size`` at a time, as
    (b, 1, N) or -- with ``dry`` -- ``lightning.stack_dry_wet``'s (b, 2, N), under ``no_grad`` and in eval mode (its mode is
    put back afterwards).  Its first output is the LFO, (b, 1, n_f) or (b, n_f); a model that returns a pair (LFO, latent) is
    accepted.  The windows' LFOs are stitched by ``stitch_lfo`` at the windows' own point rate."""
    from .lightning import stack_dry_wet
    fn = "extract_lfo_track"
    w = _file_row(wet, "wet", fn)
    L = w.numel()
    d = None
    if dry is not None:
        d = _file_row(dry, "dry", fn)
        if d.numel() != L or d.device != w.device:
            raise ValueError(f"{fn}: dry and wet must have the same length on the same device, got {d.numel()} and {L}")
    N = _int(n_samples, "n_samples", fn)
    if _int(batch_size, "batch_size", fn) < 1:
        raise ValueError(f"{fn}: batch_size must be at least 1, got {batch_size}")
    starts = window_starts(L, N, hop)
    if len(starts) > MAX_WINDOWS:
        raise ValueError(f"{fn}: {len(starts)} windows; mx_lfo_stitch takes {MAX_WINDOWS} (a larger hop)")
    hop = max(1, N // 2) if hop is None else hop
    was_training = getattr(model, "training", False)
    if hasattr(model, "eval"):
        model.eval()
    lfos = []
    try:
        with torch.no_grad():
            for i in range(0, len(starts), batch_size):
                j = min(i + batch_size, len(starts))
                wb = _windows_of(w, starts, i, j, N, hop)
                out = model(wb if d is None else stack_dry_wet(_windows_of(d, starts, i, j, N, hop), wb))
                lfo = out[0] if isinstance(out, (tuple, list)) else out
                if not isinstance(lfo, torch.Tensor) or lfo.size(0) != j - i or lfo.ndim not in (2, 3) or (
                        lfo.ndim == 3 and lfo.size(1) != 1):
                    raise ValueError(f"{fn}: the model's first output must be the LFO, (b, 1, n_f) or (b, n_f)")
                lfos.append(lfo.reshape(j - i, -1).float())
    finally:
        if was_training and hasattr(model, "train"):
            model.train()
    windows = lfos[0] if len(lfos) == 1 else torch.cat(lfos, 0)
    track, cover = stitch_lfo(windows, starts, L, N)
    return LfoTrack(track, cover, windows, starts)


def render_file(step, dry: T, track: T, fx_params=None) -> T:
    """wet_hat (L,): ``step.render`` on the file as one row of L samples, driven by ``track`` (n_t,) at its own rate -- the
    effect's state starts where the recording starts.  The effect parameters are ``step.learned_fx``'s, the fixed values
    or an explicit ``fx_params`` dict (floats, or (1,) tensors); a step with ``fx_head`` predicts them per CLIP from a latent
    a file does not have and is refused.  A one-row batch is of the step's first kind.
    The flanger kernels keep the delay line AND a low-rate LFO row in LDS (``fx.FLANGER_MAX_DELAY_SAMPLES`` floats together):
    a track that does not fit beside the step's delay line is first brought to full rate by
    ``util.linear_interpolate_last_dim`` (align_corners, the rule of the in-kernel resampling), the ``n_mod == N`` path."""
    from . import fx
    from .util import linear_interpolate_last_dim
    fn = "render_file"
    if getattr(step, "fx_head", None) is not None:
        raise ValueError(f"{fn}: a step with fx_head predicts per-clip parameters from a latent; file-level rendering with "
                         "fx_head is out of scope (use learned_fx, fixed values or fx_params)")
    d = _file_row(dry, "dry", fn)
    L = d.numel()
    if not isinstance(track, torch.Tensor) or track.ndim != 1 or track.dtype != torch.float32 or track.device != d.device:
        raise ValueError(f"{fn}: track must be an fp32 tensor of shape (n_t,) on dry's device")
    n_t = track.numel()
    if not 2 <= n_t <= L:
        raise ValueError(f"{fn}: a track of {n_t} points for {L} samples (need 2 <= n_t <= L)")
    mod = track.detach().reshape(1, n_t)
    line = step._mixed_rows(1, d.device)["max_delay_max"]
    if n_t != L and line and n_t + line > fx.FLANGER_MAX_DELAY_SAMPLES:
        mod = linear_interpolate_last_dim(mod, L, align_corners=True)
    return step.render(d.view(1, 1, L), mod.contiguous(), fx_params).reshape(L)


def fit_track(track: T, point_rate: float, rate_hz=(0.25, 8.0), rate_div: Optional[int] = None):
    """(LFOFit, points fitted): ``modulations.fit_lfo`` on the WHOLE track, whatever its length.  With ``rate_div=None`` a
    track of at most ``FIT_MAX_POINTS`` points is one ``mx_lfo_fit`` launch (K18), ``rate_div`` (default 4) lowered until its
    grid has at most ``FIT_MAX_RATES`` rates; a longer track is fitted at ``rate_div`` 4 by ``mx_track_fit`` (K23).  An explicit
    ``rate_div`` is passed on as it is, and ``modulations.fit_plan`` picks the route."""
    from .modulations import fit_lfo, fit_rate_window
    f_min, f_max = fit_rate_window(rate_hz, float(point_rate))
    n = track.numel()
    if rate_div is not None:
        return fit_lfo(track, point_rate, (f_min, f_max), rate_div=rate_div), n
    if n > FIT_MAX_POINTS:
        return fit_lfo(track, point_rate, (f_min, f_max), rate_div=4), n
    for rate_div in (4, 3, 2, 1):
        if int((f_max - f_min) / (float(point_rate) / (rate_div * n))) + 1 <= FIT_MAX_RATES:
            return fit_lfo(track[:n], point_rate, (f_min, f_max), rate_div=rate_div), n
    raise ValueError(f"fit_track: the rate window {rate_hz!r} needs more than {FIT_MAX_RATES} rates on {n} points")


def score_pair(step, model, dry: T, wet: T, lag: int = 0, polarity: int = 1, hop: Optional[int] = None,
               fit_rate_hz=(0.25, 8.0), n_samples: int = 88200, batch_size: int = 32, fx_params=None,
               rate_track: Optional[dict] = None, drift=None) -> Dict[str, object]:
    """One dry / wet recording against ``step`` (an ``LFOExtractionThroughEffect``) and its extractor ``model``:
    1. ``alignment.shift_rows`` brings ``wet`` onto ``dry`` by ``lag`` samples and ``polarity`` (+1 / -1) -- K19's convention;
    2. ``extract_lfo_track`` over windows of ``n_samples`` (``dry`` is shown too iff ``step.use_dry``);
    3. ``fit_track``: rate, shape and residual of the whole track (``fit_points`` is its number of points);
    4. ``render_file`` from the track;
    5. the match ``step`` is configured for (``match_fir`` / ``match_gain``) with the WHOLE FILE as one row: one FIR or one
       gain per file; then, with ``match_shaper``, ONE curve per file on that row (``shaper`` (K,) in the result);
    6. the terms of ``step.audio_loss_dict`` on the matched render, cut into consecutive rows of ``n_samples`` (the tail is
       dropped: every loss kernel runs at the shapes it is tested at).
    Returns device scalars and tensors: the terms by name, ``rate_hz``, ``shape`` (id of ``modulations.SHAPE_NAMES``),
    ``resid``, ``gain`` () or ``fir`` (K,) when matched, ``track`` (n_t,), ``wet_hat`` (L,), and the Python ints ``n_windows``
    and ``fit_points``.
    ``rate_track``: None, or a dict of ``rate_track.fit_rate_track`` keywords -- ``slice_points`` / ``hop_points``, or ``slice_s``
    / ``hop_s`` in seconds, converted with the track's point rate; ``rate_hz`` defaults to ``fit_rate_hz``.  The track's rate
    contour (K25) is then fitted too, the clean LFO it describes (``synth_from_rate_track``) is rendered through step 4 and
    scored by steps 5 and 6 with a match of its own, and the result gains ``rate_track`` (the ``RateTrack``), ``rate_min_hz``,
    ``rate_max_hz``, ``rate_resid`` (the mean slice residual), ``fit_wet_hat`` (L,) and ``fit/<name>`` for every term: whether a
    parametric LFO is enough to reproduce the recording.  With None nothing is added and nothing more is launched.
    ``drift``: None, an ``alignment.PairDrift`` or an ``(offset, drift)`` pair of floats (K26) -- step 1 is then
    ``alignment.warp_rows`` along that line onto ``dry``'s length instead of ``shift_rows``, so ``wet`` may have any length; a
    ``PairDrift`` brings its own polarity (``polarity`` stays +1), an untrusted one (``ok`` False) is refused, and ``lag != 0``
    beside ``drift`` is a ValueError.  The result gains the floats ``drift_ppm`` and ``lag_offset``.  With None step 1 is the
    ``shift_rows`` launch as before and nothing is added."""
    from .alignment import PairDrift, shift_rows, warp_rows
    from .effect_losses import effect_loss_terms
    fn = "score_pair"
    d, w = _file_row(dry, "dry", fn), _file_row(wet, "wet", fn)
    L, N = d.numel(), _int(n_samples, "n_samples", fn)
    if (drift is None and w.numel() != L) or w.device != d.device:
        raise ValueError(f"{fn}: dry and wet must have the same length on the same device, got {L} and {w.numel()}")
    if polarity not in (1, -1):
        raise ValueError(f"{fn}: polarity must be +1 or -1, got {polarity!r}")
    line = None
    if drift is not None:
        if _int(lag, "lag", fn) != 0:
            raise ValueError(f"{fn}: lag = {lag} beside drift: the line's offset is the lag")
        if isinstance(drift, PairDrift):
            if not drift.ok or polarity != 1:
                raise ValueError(f"{fn}: a PairDrift must be trusted (ok) and brings its own polarity; got {drift!r}, polarity = {polarity}")
            line, polarity = (float(drift.offset), float(drift.drift)), drift.polarity
        else:
            try:
                line = (float(drift[0]), float(drift[1]))
                assert len(drift) == 2
            except (TypeError, ValueError, IndexError, AssertionError):
                raise ValueError(f"{fn}: drift must be None, a PairDrift or (offset, drift), got {drift!r}") from None
    if getattr(step, "fx_head", None) is not None:
        raise ValueError(f"{fn}: file-level scoring of a step with fx_head is out of scope")
    dev = d.device
    if line is None:
        w = shift_rows(w.view(1, L), torch.full((1,), _int(lag, "lag", fn), dtype=torch.int32, device=dev),
                       torch.full((1,), float(polarity), dtype=torch.float32, device=dev)).view(L)
    else:
        w = warp_rows(w, line[0], line[1], n_out=L, polarity=polarity)
    lt = extract_lfo_track(model, w, d if step.use_dry else None, N, hop, batch_size)
    n_t = lt.track.numel()
    point_rate = float(step.sr) * (n_t - 1) / (L - 1)
    fit, fit_points = fit_track(lt.track, point_rate, fit_rate_hz)
    wet_hat = render_file(step, d, lt.track, fx_params)

    def matched_terms(wet_hat: T) -> Dict[str, object]:
        """steps 5 and 6 on one render: the terms, ``gain`` or ``fir`` when matched, and the matched ``wet_hat``"""
        out: Dict[str, object] = {}
        with torch.no_grad():
            if step.match_fir is not None:
                from .fir_match import match_fir
                m = match_fir(wet_hat.view(1, L), w.view(1, L), step.match_fir, step.match_fir_centre, step.match_fir_ridge,
                              step.match_fir_eps, step.match_fir_max_gain)
                wet_hat, out["fir"] = m.z.view(L), m.taps[0]
            elif step.match_gain is not None:
                from .gain import match_gain
                m = match_gain(wet_hat.view(1, L), w.view(1, L), step.match_gain, step.match_gain_eps, step.match_gain_range)
                wet_hat, out["gain"] = m.z.view(L), m.gain[0]
            if getattr(step, "match_shaper", None) is not None:     # ONE curve per file, on the linearly matched row (K27)
                from .shaper import match_shaper
                m = match_shaper(wet_hat.view(1, L), w.view(1, L), step.match_shaper, step.match_shaper_even,
                                 step.match_shaper_ridge, step.match_shaper_max_gain)
                wet_hat, out["shaper"] = m.z.view(L), m.coeffs[0]
            rows = L // N
            a, t = wet_hat[:rows * N].view(rows, 1, N), w[:rows * N].view(rows, 1, N)
            names = list(step.audio_loss_dict)
            if any(k in ("l1", "mse", "esr", "dc") for k in names):
                out.update({k: v for k, v in effect_loss_terms(a, t).items() if k in names})
            for k in names:
                if k not in out:
                    out[k] = step._loss_module(k)(a, t)
        out["wet_hat"] = wet_hat
        return out

    out = matched_terms(wet_hat)
    out.update(rate_hz=fit.rate_hz[0], shape=fit.shape[0], resid=fit.resid[0], track=lt.track, wet_hat=out.pop("wet_hat"),
               n_windows=len(lt.starts), fit_points=fit_points)
    if line is not None:
        out.update(drift_ppm=1e6 * line[1], lag_offset=line[0])
    if rate_track is not None:
        from .rate_track import fit_rate_track, synth_from_rate_track
        if not isinstance(rate_track, dict):
            raise ValueError(f"{fn}: rate_track must be None or a dict of fit_rate_track keywords, got {rate_track!r}")
        kw = dict(rate_track)
        for sec, pts in (("slice_s", "slice_points"), ("hop_s", "hop_points")):
            if sec in kw:
                if pts in kw:
                    raise ValueError(f"{fn}: rate_track has both {sec} and {pts}")
                kw[pts] = max(1, int(round(float(kw.pop(sec)) * point_rate)))
        if "slice_points" not in kw:
            raise ValueError(f"{fn}: rate_track needs slice_points or slice_s")
        kw.setdefault("rate_hz", fit_rate_hz)
        rt = fit_rate_track(lt.track, point_rate, **kw)
        scored = matched_terms(render_file(step, d, synth_from_rate_track(rt), fx_params))
        out.update({f"fit/{k}": scored[k] for k in step.audio_loss_dict})
        out.update(rate_track=rt, rate_min_hz=rt.rate_hz[0].min(), rate_max_hz=rt.rate_hz[0].max(),
                   rate_resid=rt.resid[0].mean(), fit_wet_hat=scored["wet_hat"])
    return out

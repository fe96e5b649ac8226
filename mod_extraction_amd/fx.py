"""Host mirror of mod_extraction/fx.py: same class, constructor and forward signature
(fx.py:25-44,121-130); the per-sample delay-line recurrence runs in the ``mx_flanger_fwd`` HIP
kernel (one wavefront per clip, delay line in LDS) instead of 88 200 python iterations.
``apply_effect`` is differentiable (``mx_flanger_fwd_stash`` + ``mx_flanger_bwd`` / ``mx_flanger_bwd_lr``) when grad mode
is on and an input requires grad; mod_sig may be full rate or the low-rate row the kernel resamples itself.  ``PhaserModule`` is the same for the phaser (``mx_phaser_fwd_stash`` + ``mx_phaser_bwd``), with the LFO
either JUCE's built-in oscillator or an external signal, on the cut-off-update grid or (``mod_sig_low_rate``) at any lower rate
(``mx_phaser_mod_expand`` / ``mx_phaser_dmod_gather``).
"""
from typing import Dict, Optional, Tuple, Union

import torch
from torch import Tensor as T, nn
from torch.autograd.function import once_differentiable

from . import _hip

Param = Union[float, T]


def delay_samples(ms: float, sr: float) -> int:
    """fx.py:40-41."""
    return int(((ms / 1000.0) * sr) + 0.5)


def apply_tremolo(x: T, mod_sig: T, mix: Param = 1.0) -> T:
    """fx.py:13-22.  An fp32 HIP x with nothing requiring grad goes through ``mx_tremolo_fwd`` (bit-identical to the
    expression below); everything else -- host tensors, other dtypes, a graph to record -- keeps the torch expression, so
    torch autograd through this function is what it was.  ``TremoloModule`` is the differentiable kernel path."""
    assert x.ndim == 3 and x.size(0) == mod_sig.size(0) and x.size(-1) == mod_sig.size(-1)
    if mod_sig.ndim == 2:
        mod_sig = mod_sig.unsqueeze(1).expand(-1, x.size(1), -1)
    if isinstance(mix, T):
        assert mix.size(0) == x.size(0)
    assert 0.0 <= mix <= 1.0                    # fx.py:21 (a tensor mix must therefore hold one element)
    graph = torch.is_grad_enabled() and any(isinstance(t, T) and t.requires_grad for t in (x, mod_sig, mix))
    if (x.is_cuda and x.dtype == torch.float32 and mod_sig.dtype == torch.float32 and mod_sig.device == x.device
            and mod_sig.shape == x.shape and not graph and (not isinstance(mix, T) or mix.dtype == torch.float32)):
        bs, n_ch, n = x.shape
        consts = derive_tremolo_constants(bs, x.device, mix, check=False)
        xr, mr = _channel_rows_of(x, mod_sig)
        y = tremolo_forward(xr, mr, {k: _per_row(v, n_ch) for k, v in consts.items()})
        return y.view(bs, n_ch, n)
    return ((1.0 - mix) * x) + (mix * mod_sig * x)


def _check_range(param: Param, bs: int, lo: float, hi: float, lo_open: bool = False, hi_open: bool = False) -> None:
    """The range check of every effect parameter: a (bs,) tensor or a float inside [lo, hi] (open ends where said)."""
    if isinstance(param, T):
        assert param.shape == (bs,)
        a, b = float(param.min()), float(param.max())
    else:
        a = b = float(param)
    assert a > lo if lo_open else a >= lo
    assert b < hi if hi_open else b <= hi


def _check_param(param: Param, bs: int, can_be_one: bool = True) -> None:
    """fx.py:46-70: all parameters >= 0; feedback < 1 strictly, the others <= 1."""
    _check_range(param, bs, 0.0, 1.0, hi_open=not can_be_one)


def derive_clip_constants(bs: int, device: torch.device, max_min_delay_samples: int,
                          max_lfo_delay_samples: int, feedback: Param, min_delay_width: Param,
                          width: Param, depth: Param, mix: Param, check: bool = True) -> Dict[str, T]:
    """Per-clip fp32 constants of fx.py:98-99,114-117, rounded where the reference rounds them: a
    tensor parameter meets the integer sample count in fp32, a python float meets it in double."""
    if check:
        _check_param(feedback, bs, can_be_one=False)
        for p in (min_delay_width, width, depth, mix):
            _check_param(p, bs)

    def vec(p: Param) -> T:
        if isinstance(p, T):
            return p.to(device=device, dtype=torch.float32).contiguous()
        return torch.full((bs,), float(p), device=device, dtype=torch.float32)

    def times_int(p: Param, k: int) -> T:
        if isinstance(p, T):
            return (vec(p) * float(k)).contiguous()
        return torch.full((bs,), float(p) * k, device=device, dtype=torch.float32)

    mix_v = vec(mix)
    omm = (1.0 - mix_v) if isinstance(mix, T) else torch.full((bs,), 1.0 - float(mix), device=device,
                                                             dtype=torch.float32)
    return {"lfo_scale": times_int(width, max_lfo_delay_samples),
            "min_delay": times_int(min_delay_width, max_min_delay_samples),
            "feedback": vec(feedback), "depth": vec(depth), "mix": mix_v, "one_minus_mix": omm.contiguous()}


def _rows_view(t: T) -> Tuple[int, int]:
    """(data_ptr, row stride in floats) of a (B, N) view whose rows are contiguous."""
    if not t.is_cuda:
        raise _hip.HipLibraryError("mod_extraction_amd ops need tensors on a HIP device (no CPU fallback)")
    assert t.dtype == torch.float32 and t.ndim == 2 and t.stride(1) == 1
    return t.data_ptr(), t.stride(0)


def _rows_arg(rows: Optional[T]) -> Tuple[Optional[int], int]:
    """The (rows, n_rows) argument pair of every launch: an optional list of clip indices to process."""
    return _hip.ptr(rows), 0 if rows is None else rows.numel()


def _per_row(v: T, n_ch: int) -> T:
    """A (bs,) per-clip vector repeated for the n_ch rows of each clip: a clip's channels share its parameters."""
    return (v.repeat_interleave(n_ch) if n_ch > 1 else v).contiguous()


def _channel_rows_of(x: T, mod_sig: T) -> Tuple[T, T]:
    """x (bs, n_ch, n) and mod_sig (bs, n_mod) / (bs, 1 | n_ch, n_mod) as the kernels' rows: one row per (clip, channel),
    (bs n_ch, n) with contiguous samples and (bs n_ch, n_mod) dense; a mod_sig without a channel axis (or with one of 1) is
    shared by its clip's channels (fx.py:84-85)."""
    bs, n_ch, n = x.shape
    xr = x.reshape(bs * n_ch, n).float()
    if xr.stride(-1) != 1:
        xr = xr.contiguous()
    if mod_sig.ndim == 2 or mod_sig.size(1) == 1:
        mod_sig = mod_sig.reshape(bs, 1, -1).expand(-1, n_ch, -1)
    return xr, mod_sig.reshape(bs * n_ch, -1).float().contiguous()


def derive_tremolo_constants(bs: int, device: torch.device, mix: Param, check: bool = True) -> Dict[str, T]:
    """The per-clip fp32 constants of fx.py:22 under the rounding rule of ``derive_clip_constants``: a tensor mix gives
    1 - mix in fp32, a python float gives it in double, rounded to fp32 once."""
    if check:
        _check_param(mix, bs)
    if isinstance(mix, T):
        mix_v = mix.to(device=device, dtype=torch.float32).contiguous()
        return {"mix": mix_v, "one_minus_mix": (1.0 - mix_v).contiguous()}
    return {"mix": torch.full((bs,), float(mix), device=device, dtype=torch.float32),
            "one_minus_mix": torch.full((bs,), 1.0 - float(mix), device=device, dtype=torch.float32)}


def tremolo_forward(x: T, mod_sig: T, consts: Dict[str, T], rows: Optional[T] = None, out: Optional[T] = None) -> T:
    """Launch mx_tremolo_fwd.  x, out: (B,N) fp32 views with contiguous rows (any row stride, e.g. one channel of a (B,2,N)
    tensor); mod_sig (B,n_mod) fp32 dense, 1 <= n_mod <= N (a shorter row is resampled in-kernel); consts from
    ``derive_tremolo_constants``; rows: optional int32 list of the rows to process (the others of ``out`` are untouched)."""
    B, N = x.shape
    assert mod_sig.ndim == 2 and mod_sig.size(0) == B and 1 <= mod_sig.size(1) <= N
    y = out if out is not None else torch.empty_like(x)
    assert y.shape == x.shape
    _hip.call("mx_tremolo_fwd", *_rows_view(x), _hip.ptr(mod_sig), mod_sig.size(1), _hip.ptr(consts["mix"]),
              _hip.ptr(consts["one_minus_mix"]), *_rows_arg(rows), B, N, *_rows_view(y), _hip.stream())
    return y


def tremolo_backward(dy: T, x: T, mod_sig: T, consts: Dict[str, T], rows: Optional[T] = None, need_dx: bool = True,
                     need_dmod: bool = True, need_dmix: bool = True,
                     dmod: Optional[T] = None, dmix: Optional[T] = None) -> Tuple[Optional[T], Optional[T], Optional[T]]:
    """Launch mx_tremolo_bwd: the adjoint of fx.py:13-22 behind the in-kernel resampling.  dy, x: (B,N) views with
    contiguous rows; mod_sig (B,n_mod) as the forward was given.  Returns dx (B,N) fp32, dmod (B,n_mod) fp32 and dmix (B,)
    fp64 (the one_minus_mix path included), each None unless asked for; rows not listed in ``rows`` hold zeros.  dmod: an
    optional (B,n_mod) dense output (e.g. a gradient shared with other effects) whose listed rows are written and whose
    other rows are not touched.  dmix: likewise an optional (B,) fp64 output (e.g. the mix row of the step's (6, B) parameter
    gradients); the kernel writes, it does not add, so the rows not listed keep what they held."""
    B, N = x.shape
    dev = x.device
    n_mod = mod_sig.size(1)
    assert mod_sig.ndim == 2 and mod_sig.size(0) == B and 1 <= n_mod <= N and dy.shape == x.shape
    if dy.stride(-1) != 1 or dy.stride(0) < N:            # e.g. the expanded ones of y.sum().backward()
        dy = dy.contiguous()
    new = torch.empty if rows is None else torch.zeros
    dx = new((B, N), device=dev, dtype=torch.float32) if need_dx else None
    if not need_dmod:
        dmod = None
    elif dmod is None:
        dmod = new((B, n_mod), device=dev, dtype=torch.float32)
    assert dmod is None or (dmod.shape == (B, n_mod) and dmod.dtype == torch.float32)
    if not need_dmix:
        dmix = None
    elif dmix is None:
        dmix = torch.zeros((B,), device=dev, dtype=torch.float64)
    assert dmix is None or (dmix.shape == (B,) and dmix.dtype == torch.float64)
    dxp, dxs = _rows_view(dx) if need_dx else (None, 0)
    _hip.call("mx_tremolo_bwd", *_rows_view(dy), *_rows_view(x), _hip.ptr(mod_sig), n_mod, _hip.ptr(consts["mix"]),
              _hip.ptr(consts["one_minus_mix"]), *_rows_arg(rows), B, N, dxp, dxs, _hip.ptr(dmod), _hip.ptr(dmix),
              _hip.stream())
    return dx, dmod, dmix


def flanger_forward(x: T, mod_sig: T, consts: Dict[str, T], max_delay: T, max_delay_max: int,
                    rows: Optional[T] = None, out: Optional[T] = None, mod_up: Optional[T] = None,
                    dbg_prev: Optional[T] = None, dbg_frac: Optional[T] = None) -> T:
    """Launch mx_flanger_fwd.  x, out: (B,N) fp32 views with contiguous rows (any row stride, e.g. one
    channel of a (B,2,N) tensor); mod_sig (B,n_mod) fp32; max_delay (B,) int32."""
    B, N = x.shape
    y = out if out is not None else torch.empty_like(x)
    _hip.call("mx_flanger_fwd", *_rows_view(x), _hip.ptr(mod_sig), mod_sig.size(-1),
              _hip.ptr(consts["lfo_scale"]), _hip.ptr(consts["min_delay"]), _hip.ptr(consts["feedback"]),
              _hip.ptr(consts["depth"]), _hip.ptr(consts["mix"]), _hip.ptr(consts["one_minus_mix"]),
              _hip.ptr(max_delay), int(max_delay_max), *_rows_arg(rows),
              B, N, *_rows_view(y), _hip.ptr(mod_up), _hip.ptr(dbg_prev), _hip.ptr(dbg_frac), _hip.stream())
    return y


def flanger_forward_stash(x: T, mod_sig: T, consts: Dict[str, T], max_delay: T, max_delay_max: int,
                          rows: Optional[T] = None, out: Optional[T] = None,
                          stash: Optional[T] = None) -> Tuple[T, T]:
    """Launch mx_flanger_fwd_stash: ``flanger_forward`` (same y, bit for bit) that also returns the tap v[n] of fx.py:113 of
    every sample, (B,N) dense, for ``flanger_backward``.  mod_sig (B,n_mod), n_mod == N or shorter (resampled in-kernel)."""
    B, N = x.shape
    assert mod_sig.ndim == 2 and mod_sig.size(0) == B and 1 <= mod_sig.size(1) <= N
    y = out if out is not None else torch.empty_like(x)
    st = stash if stash is not None else torch.empty((B, N), device=x.device, dtype=torch.float32)
    _hip.call("mx_flanger_fwd_stash", *_rows_view(x), _hip.ptr(mod_sig), mod_sig.size(1),
              _hip.ptr(consts["lfo_scale"]), _hip.ptr(consts["min_delay"]), _hip.ptr(consts["feedback"]),
              _hip.ptr(consts["depth"]), _hip.ptr(consts["mix"]), _hip.ptr(consts["one_minus_mix"]),
              _hip.ptr(max_delay), int(max_delay_max), *_rows_arg(rows),
              B, N, *_rows_view(y), _hip.ptr(st), _hip.stream())
    return y, st


PARAM_GRADS = ("lfo_scale", "min_delay", "feedback", "depth", "mix")
FLANGER_MAX_DELAY_SAMPLES = 34784      # csrc/flanger_common.h FL_MAX_M: delay line + a resampled LFO row, in LDS


def _param_grad_outputs(names: Tuple[str, ...], given: Optional[Dict[str, T]], B: int, dev) -> Dict[str, T]:
    """The (B,) fp64 outputs of an adjoint's parameter gradients: the caller's where given, else fresh zeros."""
    out = {}
    for k in names:
        g = None if given is None else given.get(k)
        if g is None:
            g = torch.zeros((B,), device=dev, dtype=torch.float64)
        assert g.shape == (B,) and g.dtype == torch.float64 and g.is_contiguous(), k
        out[k] = g
    return out


def flanger_backward(dy: T, x: T, mod_sig: T, stash: T, consts: Dict[str, T], max_delay: T, max_delay_max: int,
                     rows: Optional[T] = None, need_dx: bool = True, need_dmod: bool = True,
                     params: Tuple[str, ...] = PARAM_GRADS, dx: Optional[T] = None,
                     dmod: Optional[T] = None,
                     grads: Optional[Dict[str, T]] = None) -> Tuple[Optional[T], Optional[T], Dict[str, T]]:
    """Launch mx_flanger_bwd (mod_sig at full rate) or mx_flanger_bwd_lr (a shorter mod_sig, as the stash forward was
    given): the adjoint of fx.py:72-119 (the gradient the DESIGN K-table row defines).
    dy, x: (B,N) views with contiguous rows; stash (B,N) and mod_sig (B,n_mod) dense.  Returns dx (B,N), dmod (B,n_mod)
    (None unless asked for) and the per-clip fp64 gradients of the constants named in ``params`` (d mix includes the
    one_minus_mix path).  grads: optional (B,) fp64 outputs by name for (some of) ``params`` (e.g. rows of the step's (6, B)
    parameter gradients) instead of fresh zeros; the kernel writes, it does not add, so rows not listed keep what they held."""
    B, N = x.shape
    dev = x.device
    n_mod = mod_sig.size(1)
    assert mod_sig.ndim == 2 and mod_sig.size(0) == B and 1 <= n_mod <= N
    if dy.stride(-1) != 1 or dy.stride(0) < N:            # e.g. the expanded ones of y.sum().backward()
        dy = dy.contiguous()
    if need_dx and dx is None:
        dx = torch.empty((B, N), device=dev, dtype=torch.float32)
    if need_dmod and dmod is None:
        dmod = torch.empty((B, n_mod), device=dev, dtype=torch.float32)
    assert not need_dmod or dmod.size(1) == n_mod
    dxp, dxs = _rows_view(dx) if need_dx else (None, 0)
    dmp, dms = _rows_view(dmod) if need_dmod else (None, 0)
    grads = _param_grad_outputs(params, grads, B, dev)
    ws = torch.empty((B, N), device=dev, dtype=torch.float32)
    entry = ("mx_flanger_bwd", ()) if n_mod == N else ("mx_flanger_bwd_lr", (n_mod,))
    _hip.call(entry[0], *_rows_view(dy), *_rows_view(x), _hip.ptr(mod_sig), *entry[1], _hip.ptr(stash),
              _hip.ptr(consts["lfo_scale"]), _hip.ptr(consts["min_delay"]), _hip.ptr(consts["feedback"]),
              _hip.ptr(consts["depth"]), _hip.ptr(consts["mix"]), _hip.ptr(consts["one_minus_mix"]),
              _hip.ptr(max_delay), int(max_delay_max), *_rows_arg(rows), B, N,
              _hip.ptr(ws), dxp, dxs, dmp, dms, *[_hip.ptr(grads.get(k)) for k in PARAM_GRADS], _hip.stream())
    return (dx if need_dx else None), (dmod if need_dmod else None), grads


class _FlangerFunction(torch.autograd.Function):
    """y = flanger(x, mod, constants) over (clip, channel) rows; the (bs,) constants are shared by a clip's n_ch rows, so
    their gradients are summed over the channels (in fp64) before they are rounded to the constants' dtype."""

    @staticmethod
    def forward(ctx, x, mod_sig, lfo_scale, min_delay, feedback, depth, mix, one_minus_mix, n_ch, max_delay_samples):
        rows = x.size(0)
        consts = {"lfo_scale": lfo_scale, "min_delay": min_delay, "feedback": feedback, "depth": depth, "mix": mix,
                  "one_minus_mix": one_minus_mix}
        consts = {k: _per_row(v.detach(), n_ch) for k, v in consts.items()}
        md = torch.full((rows,), max_delay_samples, device=x.device, dtype=torch.int32)
        y, stash = flanger_forward_stash(x.detach(), mod_sig.detach(), consts, md, max_delay_samples)
        ctx.save_for_backward(x, mod_sig, stash)
        ctx.consts, ctx.md, ctx.n_ch, ctx.max_delay_samples = consts, md, n_ch, max_delay_samples
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, mod_sig, stash = ctx.saved_tensors
        need = ctx.needs_input_grad
        params = tuple(k for k, n in zip(PARAM_GRADS, need[2:7]) if n)
        dx, dmod, g = flanger_backward(dy, x, mod_sig, stash, ctx.consts, ctx.md, ctx.max_delay_samples,
                                       need_dx=need[0], need_dmod=need[1], params=params)
        out = [dx, dmod]
        for k in PARAM_GRADS:
            out.append(g[k].view(-1, ctx.n_ch).sum(1).float() if k in g else None)
        return tuple(out) + (None, None, None)


class MonoFlangerChorusModule(nn.Module):
    def __init__(self, batch_size: int, n_ch: int, n_samples: int, sr: float,
                 max_min_delay_ms: float, max_lfo_delay_ms: float) -> None:
        super().__init__()
        assert n_ch >= 1
        self.batch_size = batch_size
        self.n_ch = n_ch
        self.n_samples = n_samples
        self.sr = sr
        self.max_min_delay_ms = max_min_delay_ms
        self.max_lfo_delay_ms = max_lfo_delay_ms
        self.max_min_delay_samples = delay_samples(max_min_delay_ms, sr)
        self.max_lfo_delay_samples = delay_samples(max_lfo_delay_ms, sr)
        self.max_delay_samples = self.max_min_delay_samples + self.max_lfo_delay_samples
        # the reference registers delay_buf / out_buf buffers (fx.py:43-44); here the delay line
        # lives in LDS for the duration of the kernel and the output is the returned tensor.

    def check_param(self, param: Param, bs: int, out_n_dim: int = 2, can_be_one: bool = True) -> Param:
        """fx.py:46-70: range check of one effect parameter ((bs,) tensor or float in [0, 1], or [0, 1) when it may not be
        one) and its broadcast view; ``forward`` applies the same checks inside ``derive_clip_constants``."""
        _check_param(param, bs, can_be_one)
        if not isinstance(param, T):
            return param
        if out_n_dim not in (2, 3):
            raise ValueError
        return param.view((-1,) + (1,) * (out_n_dim - 1))

    def apply_effect(self, x: T, mod_sig: T, feedback: Param, min_delay_width: Param, width: Param, depth: Param,
                     mix: Param) -> T:
        """fx.py:72-119 (the per-sample loop) = one kernel launch here; ``forward`` is this under no_grad, as in the
        reference.  With grad mode on and x, mod_sig or a tensor parameter requiring grad, the output carries a grad_fn
        (``mx_flanger_fwd_stash`` forward, ``mx_flanger_bwd`` backward; y is the same, bit for bit).  mod_sig is full rate
        or any shorter row, which the kernel resamples as ``forward`` does (``mx_flanger_bwd_lr`` backward): its gradient has
        mod_sig's own shape.  Python-float parameters get no gradient."""
        params = (feedback, min_delay_width, width, depth, mix)
        if torch.is_grad_enabled() and (x.requires_grad or mod_sig.requires_grad or
                                        any(isinstance(p, T) and p.requires_grad for p in params)):
            return self._apply_effect_grad(x, mod_sig, *params)
        return self.forward(x, mod_sig, feedback, min_delay_width, width, depth, mix)

    def _prepare(self, x: T, mod_sig: T, feedback: Param, min_delay_width: Param, width: Param, depth: Param,
                 mix: Param):
        """The checks, the per-clip constants and the rows both paths launch on.  n_ch > 1 (fx.py:81-85,104-115): every
        channel owns a delay line = one kernel row per (clip, channel); a clip's channels share its parameters (the (bs,)
        constants are returned as they are); mod_sig (bs, n) / (bs, 1, n) is shared by the channels."""
        assert x.ndim == 3
        bs, n_ch, n = x.shape
        assert n_ch == self.n_ch
        assert mod_sig.size(0) == bs
        if mod_sig.ndim == 3:
            assert mod_sig.size(1) in (1, n_ch)
        consts = derive_clip_constants(bs, x.device, self.max_min_delay_samples, self.max_lfo_delay_samples,
                                       feedback, min_delay_width, width, depth, mix)
        xr, mr = _channel_rows_of(x, mod_sig)                       # fx.py:84-85: mod_sig shared by the channels
        return xr, mr, consts, (bs, n_ch, n)

    def _apply_effect_grad(self, x: T, mod_sig: T, feedback: Param, min_delay_width: Param, width: Param, depth: Param,
                           mix: Param) -> T:
        xr, mr, consts, shape = self._prepare(x, mod_sig, feedback, min_delay_width, width, depth, mix)
        y = _FlangerFunction.apply(xr, mr, consts["lfo_scale"], consts["min_delay"], consts["feedback"], consts["depth"],
                                   consts["mix"], consts["one_minus_mix"], self.n_ch, self.max_delay_samples)
        return y.view(shape)

    def forward(self, x: T, mod_sig: T, feedback: Param = 0.0, min_delay_width: Param = 1.0,
                width: Param = 1.0, depth: Param = 1.0, mix: Param = 1.0) -> T:
        with torch.no_grad():
            xr, mr, consts, shape = self._prepare(x, mod_sig, feedback, min_delay_width, width, depth, mix)
            consts = {k: _per_row(v, self.n_ch) for k, v in consts.items()}
            md = torch.full((xr.size(0),), self.max_delay_samples, device=x.device, dtype=torch.int32)
            y = flanger_forward(xr, mr, consts, md, self.max_delay_samples)
        return y.view(shape)


def phaser_forward(src: T, params: Dict[str, T], lead: Optional[T], sr: float, n_samples: int,
                   rows: Optional[T] = None, out: Optional[T] = None, dry_out: Optional[T] = None,
                   exact_order: bool = False) -> T:
    """Launch mx_phaser_fwd (pedalboard.Phaser semantics, datasets.py:455-482).
    src (B, >= lead+n_samples) source audio rows; params: rate_hz, depth, centre_frequency_hz,
    feedback, mix -- each (B,) fp32 on the device; lead (B,) int32 warm-up samples or None;
    out / dry_out: (B, n_samples) views with contiguous rows.  exact_order=True runs every sample in JUCE's
    operation order on one wavefront per clip (the bit reference, ~20x slower); the default is the time-parallel scan."""
    B = src.size(0)
    y = out if out is not None else torch.empty((B, n_samples), device=src.device, dtype=torch.float32)
    sp, ss = _rows_view(src)
    yp, ys = _rows_view(y)
    dp = None
    if dry_out is not None:
        dp, ds = _rows_view(dry_out)
        assert ds == ys
    # cut-off workspace of the scan kernel: one float per 4-sample group of the longest possible render (lead + n_samples
    # never exceeds a source row)
    n_items = B if rows is None else rows.numel()
    ws_stride = (src.size(-1) + 3) // 4
    ws = None if exact_order else torch.empty((n_items, ws_stride), device=src.device, dtype=torch.float32)
    _hip.call("mx_phaser_fwd", sp, ss, _hip.ptr(params["rate_hz"]), _hip.ptr(params["depth"]),
              _hip.ptr(params["centre_frequency_hz"]), _hip.ptr(params["feedback"]), _hip.ptr(params["mix"]),
              _hip.ptr(lead), *_rows_arg(rows), B, n_samples, float(sr),
              1 if exact_order else 0, yp, ys, dp, _hip.ptr(ws), ws_stride, _hip.stream())
    return y


PHASER_PARAM_GRADS = ("depth", "centre_frequency_hz", "feedback", "mix")
_PS_P, _PS_MV, _PS_SUB = 512, 57, 2                 # csrc/phaser_common.h


def derive_phaser_params(bs: int, device: torch.device, depth: Param, centre_frequency_hz: Param, feedback: Param,
                         mix: Param, check: bool = True) -> Dict[str, T]:
    """The per-clip (bs,) fp32 parameter dict of the phaser launches (no ``rate_hz``: for an external LFO) from python
    floats or (bs,) tensors; ``check``: ``PhaserModule``'s ranges (host synchronisations for tensors)."""
    if check:
        _check_range(depth, bs, 0.0, 1.0)
        _check_range(mix, bs, 0.0, 1.0)
        _check_range(feedback, bs, -1.0, 1.0, lo_open=True, hi_open=True)
        _check_range(centre_frequency_hz, bs, 0.0, float("inf"), lo_open=True)

    def vec(p: Param) -> T:
        if isinstance(p, T):
            assert p.shape == (bs,)
            return p.to(device=device, dtype=torch.float32).contiguous()
        return torch.full((bs,), float(p), device=device, dtype=torch.float32)

    return {"depth": vec(depth), "centre_frequency_hz": vec(centre_frequency_hz), "feedback": vec(feedback),
            "mix": vec(mix)}


def phaser_stash_shape(width: int) -> Tuple[int, int]:
    """(stash_groups, floats per stash row) for source rows of ``width`` samples (csrc/phaser_common.h)."""
    sg = ((width + 3) // 4 + 3) // 4 * 4
    gpc = (sg + _PS_P - 1) // _PS_P
    return sg, 4 * sg + _PS_P * _PS_MV + _PS_P * 8 * ((gpc + _PS_SUB - 1) // _PS_SUB)


def phaser_forward_stash(src: T, params: Dict[str, T], lead: Optional[T], sr: float, n_samples: int,
                         mod: Optional[T] = None, rows: Optional[T] = None, out: Optional[T] = None,
                         dry_out: Optional[T] = None, stash: Optional[T] = None) -> Tuple[T, T]:
    """Launch mx_phaser_fwd_stash: ``phaser_forward`` (the scan; same y and dry_out, bit for bit, when ``mod`` is None) that
    also returns the stash ``phaser_backward`` needs.  mod (B, n_mod >= ceil(W / 4)) fp32 dense: an
    external LFO in [0, 1], one value per cut-off update (4 samples), in the convention of the reference's phaser ground
    truth ``make_mod_signal(.., pi / 2, "cos")`` (osc = 1 - 2 mod); params["rate_hz"] is then not needed.  lead + n_samples must not exceed
    a source row (asserted here: the kernel would skip such a clip without an error)."""
    B, W = src.shape
    total = n_samples + (0 if lead is None else int(lead.max()))
    assert total <= W, "lead + n_samples exceeds a source row (the kernel would leave such a clip alone)"
    if mod is not None:
        assert mod.size(1) >= (W + 3) // 4, "mod: one value per 4 samples of a source row (any lead fits)"
    y = out if out is not None else torch.empty((B, n_samples), device=src.device, dtype=torch.float32)
    sp, ss = _rows_view(src)
    yp, ys = _rows_view(y)
    dp = None
    if dry_out is not None:
        dp, ds = _rows_view(dry_out)
        assert ds == ys
    sg, row = phaser_stash_shape(W)
    st = stash if stash is not None else torch.empty((B, row), device=src.device, dtype=torch.float32)
    assert st.shape == (B, row) and st.dtype == torch.float32
    if mod is not None:
        assert mod.ndim == 2 and mod.size(0) == B and mod.dtype == torch.float32
    _hip.call("mx_phaser_fwd_stash", sp, ss, W, _hip.ptr(mod), 0 if mod is None else mod.size(1),
              _hip.ptr(params.get("rate_hz")), _hip.ptr(params["depth"]), _hip.ptr(params["centre_frequency_hz"]),
              _hip.ptr(params["feedback"]), _hip.ptr(params["mix"]), _hip.ptr(lead), *_rows_arg(rows),
              B, n_samples, float(sr), yp, ys, dp, _hip.ptr(st), sg, row, _hip.stream())
    return y, st


def phaser_backward(dy: T, src: T, stash: T, params: Dict[str, T], lead: Optional[T], sr: float, n_samples: int,
                    rows: Optional[T] = None, need_dx: bool = True, need_dmod: bool = True,
                    params_wanted: Tuple[str, ...] = PHASER_PARAM_GRADS, dx: Optional[T] = None,
                    dmod: Optional[T] = None,
                    grads: Optional[Dict[str, T]] = None) -> Tuple[Optional[T], Optional[T], Dict[str, T]]:
    """Launch mx_phaser_bwd: the adjoint of the phaser recurrence (the gradient the DESIGN K3b row defines).
    dy (B, n_samples) and src (B, W) views with contiguous rows; stash from ``phaser_forward_stash`` on the same src, params,
    lead.  Returns dx (B, W): the gradient with respect to every processed source sample, the lead included, zeros beyond
    lead + n_samples; dmod (B, ceil(W / 4)): with respect to the external LFO (with the built-in oscillator: with respect to
    (1 - osc) / 2) (both None unless asked for); and the per-clip fp64 gradients of the parameters named in
    ``params_wanted``.  There is no gradient with respect to rate_hz.  grads: optional (B,) fp64 outputs by name, as in
    ``flanger_backward`` (written, not added to)."""
    B, W = src.shape
    dev = src.device
    if dy.stride(-1) != 1 or dy.stride(0) < n_samples:      # e.g. the expanded ones of y.sum().backward()
        dy = dy.contiguous()
    assert dy.shape == (B, n_samples)
    assert n_samples + (0 if lead is None else int(lead.max())) <= W, "lead + n_samples exceeds a source row"
    n_mod = (W + 3) // 4
    if need_dx and dx is None:
        dx = torch.empty((B, W), device=dev, dtype=torch.float32)
    if need_dmod and dmod is None:
        dmod = torch.empty((B, n_mod), device=dev, dtype=torch.float32)
    dxp, dxs = _rows_view(dx) if need_dx else (None, 0)
    dmp, dms = _rows_view(dmod) if need_dmod else (None, 0)
    assert not need_dx or dx.size(1) == W
    assert not need_dmod or dmod.size(1) >= n_mod                 # every group of the longest possible clip
    sg, row = phaser_stash_shape(W)
    assert stash.shape == (B, row)
    grads = _param_grad_outputs(params_wanted, grads, B, dev)
    _hip.call("mx_phaser_bwd", *_rows_view(dy), *_rows_view(src), W, _hip.ptr(stash), sg, row, _hip.ptr(params["depth"]),
              _hip.ptr(params["centre_frequency_hz"]), _hip.ptr(params["feedback"]), _hip.ptr(params["mix"]),
              _hip.ptr(lead), *_rows_arg(rows), B, n_samples, float(sr), dxp, dxs,
              dmp, dms, dmod.size(1) if need_dmod else 0, *[_hip.ptr(grads.get(k)) for k in PHASER_PARAM_GRADS],
              _hip.stream())
    return (dx if need_dx else None), (dmod if need_dmod else None), grads


def phaser_mod_expand(mod_lr: T, lead: Optional[T], n_samples: int, width: int, out: Optional[T] = None,
                      rows: Optional[T] = None) -> T:
    """Launch mx_phaser_mod_expand: a low-rate LFO (B, n_mod), 1 <= n_mod <= n_samples, spanning the n_samples of the clip
    window, as the (B, ceil(width / 4)) row ``phaser_forward_stash`` takes as ``mod``: group g of row b reads the row
    resampled (as ``flanger_forward`` / ``tremolo_forward`` resample theirs) at clip sample
    clamp(4 g - lead[b], 0, n_samples - 1) -- the LFO is held at its first value through the lead-in; groups beyond
    lead[b] + n_samples hold 0.5.  rows: optional int32 list of the rows to process (mx_phaser_mod_expand_rows): the listed
    rows get the same bits, the others of ``out`` are not touched (without ``out`` they are uninitialised); an empty list
    launches nothing."""
    B, n_mod = mod_lr.shape
    assert mod_lr.dtype == torch.float32 and mod_lr.is_contiguous() and 1 <= n_mod <= n_samples <= width
    ng = (width + 3) // 4
    mod_g = out if out is not None else torch.empty((B, ng), device=mod_lr.device, dtype=torch.float32)
    assert mod_g.size(0) == B and mod_g.size(1) >= ng
    mp, ms = _rows_view(mod_g)
    if rows is None:
        _hip.call("mx_phaser_mod_expand", _hip.ptr(mod_lr), n_mod, _hip.ptr(lead), B, n_samples, width, mp, ms, _hip.stream())
    elif rows.numel():
        assert rows.dtype == torch.int32 and rows.numel() <= B
        _hip.call("mx_phaser_mod_expand_rows", _hip.ptr(mod_lr), n_mod, _hip.ptr(lead), *_rows_arg(rows), B, n_samples, width,
                  mp, ms, _hip.stream())
    return mod_g


def phaser_dmod_gather(dmod_g: T, lead: Optional[T], n_samples: int, n_mod: int, rows: Optional[T] = None,
                       out: Optional[T] = None) -> T:
    """Launch mx_phaser_dmod_gather, the transpose of ``phaser_mod_expand``: dmod_g (B, >= ceil(n_samples / 4)) as
    ``phaser_backward`` returns it -> (B, n_mod) fp32 (fp64 sums in a fixed order, rounded once; deterministic).  rows:
    optional int32 list of the rows to process (mx_phaser_dmod_gather_rows): same bits on the listed rows, the others of
    ``out`` (B, n_mod) dense -- e.g. a gradient shared with other effects -- are not touched (without ``out`` they are
    uninitialised); an empty list launches nothing."""
    B = dmod_g.size(0)
    assert 1 <= n_mod <= n_samples
    dp, ds = _rows_view(dmod_g)
    dmod_lr = out if out is not None else torch.empty((B, n_mod), device=dmod_g.device, dtype=torch.float32)
    assert dmod_lr.shape == (B, n_mod) and dmod_lr.dtype == torch.float32
    if rows is None:
        _hip.call("mx_phaser_dmod_gather", dp, ds, dmod_g.size(1), _hip.ptr(lead), B, n_samples, n_mod, _hip.ptr(dmod_lr),
                  _hip.stream())
    elif rows.numel():
        assert rows.dtype == torch.int32 and rows.numel() <= B
        _hip.call("mx_phaser_dmod_gather_rows", dp, ds, dmod_g.size(1), _hip.ptr(lead), *_rows_arg(rows), B, n_samples, n_mod,
                  _hip.ptr(dmod_lr), _hip.stream())
    return dmod_lr


def phaser_forward_stash_lr(src: T, params: Dict[str, T], lead: Optional[T], sr: float, n_samples: int,
                            mod_lr: T, rows: Optional[T] = None, out: Optional[T] = None,
                            stash: Optional[T] = None) -> Tuple[T, T, T]:
    """``phaser_forward_stash`` driven by a low-rate LFO: mod_lr (B, n_mod) fp32, any 1 <= n_mod <= n_samples, spanning the
    n_samples OUTPUT samples (the lead-in holds its first value).  Two launches: ``phaser_mod_expand``, then the stash
    forward on the expanded row.  Returns (y, stash, mod_g): mod_g (B, ceil(W / 4)) is the row the scan read.  rows:
    optional int32 list of the rows to process, through both launches: the other rows of ``out`` (e.g. the wet_hat a batch
    of mixed effects shares) are not touched, those of stash and mod_g are uninitialised; an empty list launches nothing."""
    mod_g = phaser_mod_expand(mod_lr, lead, n_samples, src.size(1), rows=rows)
    if rows is not None and rows.numel() == 0:
        B = src.size(0)
        y = out if out is not None else torch.empty((B, n_samples), device=src.device, dtype=torch.float32)
        st = stash if stash is not None else torch.empty((B, phaser_stash_shape(src.size(1))[1]), device=src.device,
                                                         dtype=torch.float32)
        return y, st, mod_g
    y, stash = phaser_forward_stash(src, params, lead, sr, n_samples, mod=mod_g, rows=rows, out=out, stash=stash)
    return y, stash, mod_g


def phaser_backward_lr(dy: T, src: T, stash: T, params: Dict[str, T], lead: Optional[T], sr: float, n_samples: int,
                       n_mod: int, need_dx: bool = True, params_wanted: Tuple[str, ...] = PHASER_PARAM_GRADS,
                       rows: Optional[T] = None, dmod: Optional[T] = None,
                       grads: Optional[Dict[str, T]] = None) -> Tuple[Optional[T], T, Dict[str, T]]:
    """The adjoint of ``phaser_forward_stash_lr``: ``phaser_backward`` (dmod at group rate), then ``phaser_dmod_gather``.
    Returns (dx (B, W) or None, dmod_lr (B, n_mod), the per-clip fp64 parameter gradients named in ``params_wanted``).
    rows: the list the forward was given, through both launches; dmod: an optional (B, n_mod) dense output whose listed
    rows are written and whose other rows are not touched (without it they are uninitialised, as are those of dx); an
    empty list launches nothing.  grads: as in ``phaser_backward``."""
    if rows is not None and rows.numel() == 0:
        B, W = src.shape
        dx = torch.empty((B, W), device=src.device, dtype=torch.float32) if need_dx else None
        out = dmod if dmod is not None else torch.empty((B, n_mod), device=src.device, dtype=torch.float32)
        return dx, out, _param_grad_outputs(params_wanted, grads, B, src.device)
    dx, dmod_g, grads = phaser_backward(dy, src, stash, params, lead, sr, n_samples, rows=rows, need_dx=need_dx,
                                        need_dmod=True, params_wanted=params_wanted, grads=grads)
    return dx, phaser_dmod_gather(dmod_g, lead, n_samples, n_mod, rows=rows, out=dmod), grads


class _PhaserFunction(torch.autograd.Function):
    """y = phaser(x, mod | rate, parameters) over (clip, channel) rows; the (bs,) parameters are shared by a clip's n_ch
    rows, so their gradients are summed over the channels (in fp64) before they are rounded to the parameters' dtype."""

    @staticmethod
    def forward(ctx, x, mod, rate, depth, centre, feedback, mix, lead, n_ch, sr, n):
        def rows_of(v):
            return _per_row(v.detach().float(), n_ch)

        params = {"depth": rows_of(depth), "centre_frequency_hz": rows_of(centre), "feedback": rows_of(feedback),
                  "mix": rows_of(mix)}
        if rate is not None:
            params["rate_hz"] = rows_of(rate)
        y, stash = phaser_forward_stash(x.detach(), params, lead, sr, n, mod=None if mod is None else mod.detach())
        ctx.save_for_backward(x, stash)
        ctx.params, ctx.lead, ctx.n_ch, ctx.sr, ctx.n, ctx.has_mod = params, lead, n_ch, sr, n, mod is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, stash = ctx.saved_tensors
        need = ctx.needs_input_grad
        wanted = tuple(k for k, n in zip(PHASER_PARAM_GRADS, need[3:7]) if n)
        need_dmod = ctx.has_mod and need[1]
        dx, dmod, g = phaser_backward(dy, x, stash, ctx.params, ctx.lead, ctx.sr, ctx.n, need_dx=need[0],
                                      need_dmod=need_dmod, params_wanted=wanted)
        out = [dx, dmod, None]
        for k in PHASER_PARAM_GRADS:
            out.append(g[k].view(-1, ctx.n_ch).sum(1).float() if k in g else None)
        return tuple(out) + (None, None, None, None)


class _PhaserLowRateFunction(torch.autograd.Function):
    """``_PhaserFunction`` with the LFO at a low rate: mod (rows, n_mod) spans the n output samples
    (``phaser_forward_stash_lr`` / ``phaser_backward_lr``); the group-rate row does not outlive the forward."""

    @staticmethod
    def forward(ctx, x, mod, depth, centre, feedback, mix, lead, n_ch, sr, n):
        def rows_of(v):
            return _per_row(v.detach().float(), n_ch)

        params = {"depth": rows_of(depth), "centre_frequency_hz": rows_of(centre), "feedback": rows_of(feedback),
                  "mix": rows_of(mix)}
        y, stash, _ = phaser_forward_stash_lr(x.detach(), params, lead, sr, n, mod.detach())
        ctx.save_for_backward(x, stash)
        ctx.params, ctx.lead, ctx.n_ch, ctx.sr, ctx.n, ctx.n_mod = params, lead, n_ch, sr, n, mod.size(1)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, stash = ctx.saved_tensors
        need = ctx.needs_input_grad
        wanted = tuple(k for k, n in zip(PHASER_PARAM_GRADS, need[2:6]) if n)
        if need[1]:
            dx, dmod, g = phaser_backward_lr(dy, x, stash, ctx.params, ctx.lead, ctx.sr, ctx.n, ctx.n_mod, need_dx=need[0],
                                             params_wanted=wanted)
        else:
            dx, dmod, g = phaser_backward(dy, x, stash, ctx.params, ctx.lead, ctx.sr, ctx.n, need_dx=need[0],
                                          need_dmod=False, params_wanted=wanted)
        out = [dx, dmod]
        for k in PHASER_PARAM_GRADS:
            out.append(g[k].view(-1, ctx.n_ch).sum(1).float() if k in g else None)
        return tuple(out) + (None, None, None, None)


class PhaserModule(nn.Module):
    """The phaser of the data pipeline (pedalboard.Phaser = JUCE dsp::Phaser semantics, ``phaser_forward``) as a module in
    the shape of ``MonoFlangerChorusModule``; the reference has no counterpart (its phaser is pedalboard's, on the CPU,
    without a gradient).

    x (bs, n_ch, lead + n): the channels are rows that share their clip's parameters.  ``lead`` warm-up samples are
    processed before the n output samples (None: 0; an int; or a (bs,) integer tensor, n = width - max(lead)); the output
    is (bs, n_ch, n).  Exactly one of ``mod_sig`` and ``rate_hz`` drives the cut-off:
    * rate_hz (float or (bs,)): JUCE's built-in sine oscillator, phase 0 at sample 0;
    * mod_sig, values in [0, 1], in the convention of the reference's phaser ground truth
      ``make_mod_signal(.., pi / 2, "cos")`` = (1 + sin wt) / 2, so that JUCE's osc = 1 - 2 mod: (bs, ceil(width / 4)), one value per cut-off update, or full rate
      (bs, width), which is sampled at samples 0, 4, 8, ...; optionally with a channel axis of 1 or n_ch.
      With ``mod_sig_low_rate=True`` it is instead (bs, n_mod) (or with a channel axis of 1 or n_ch) at any 1 <= n_mod <= n
      and spans the n OUTPUT samples, resampled as the flanger and the tremolo resample theirs (align_corners=True,
      ``mx_phaser_mod_expand``); through the lead-in the LFO holds its first value.  Gradients as on the default path, the
      one of mod_sig at its own rate (``mx_phaser_dmod_gather``).
    depth, mix in [0, 1], feedback in (-1, 1) (JUCE's range), centre_frequency_hz > 0 (centres outside 20 Hz .. 20 kHz
    clamp): python floats or (bs,) tensors.

    ``forward`` runs under no_grad (bit-identical to ``phaser_forward`` when rate_hz is given).  ``apply_effect`` carries a
    grad_fn when grad mode is on and x, mod_sig or a tensor parameter requires grad (``mx_phaser_fwd_stash`` forward,
    ``mx_phaser_bwd`` backward); python-float parameters get no gradient.  There is deliberately NO gradient with respect
    to rate_hz (a rate_hz that requires grad raises): the phase is tens of thousands of sequential fp32 additions with
    wrap-around and its derivative with respect to the rate grows linearly in time, which is of no use to an optimiser; to
    fit a rate, build the LFO in torch and pass it as mod_sig."""

    def __init__(self, sr: float) -> None:
        super().__init__()
        self.sr = sr

    def _prepare(self, x: T, mod_sig: Optional[T], rate_hz: Optional[Param], depth: Param, centre_frequency_hz: Param,
                 feedback: Param, mix: Param, lead, low_rate: bool = False):
        assert x.ndim == 3
        bs, n_ch, W = x.shape
        assert (mod_sig is None) != (rate_hz is None), "exactly one of mod_sig and rate_hz"
        _check_range(depth, bs, 0.0, 1.0)
        _check_range(mix, bs, 0.0, 1.0)
        _check_range(feedback, bs, -1.0, 1.0, lo_open=True, hi_open=True)
        _check_range(centre_frequency_hz, bs, 0.0, float("inf"), lo_open=True)
        if isinstance(rate_hz, T) and rate_hz.requires_grad:
            raise ValueError("PhaserModule has no gradient with respect to rate_hz: pass the LFO as mod_sig instead")
        dev = x.device
        rows = bs * n_ch
        if lead is None:
            lead_rows, n = None, W
        elif isinstance(lead, T):
            assert lead.shape == (bs,) and not lead.is_floating_point() and int(lead.min()) >= 0
            n = W - int(lead.max())
            lead_rows = _per_row(lead.to(device=dev, dtype=torch.int32), n_ch)
        else:
            assert 0 <= int(lead) < W
            n = W - int(lead)
            lead_rows = torch.full((rows,), int(lead), device=dev, dtype=torch.int32)
        assert n > 0

        def vec(p: Param) -> T:
            if isinstance(p, T):
                assert p.shape == (bs,)
                return p.to(dev)
            return torch.full((bs,), float(p), device=dev, dtype=torch.float32)

        xr = x.reshape(rows, W).float()
        if xr.stride(-1) != 1:
            xr = xr.contiguous()
        mr = None
        if low_rate:
            assert mod_sig is not None, "mod_sig_low_rate needs a mod_sig"
            assert mod_sig.size(0) == bs and mod_sig.ndim in (2, 3) and 1 <= mod_sig.size(-1) <= n
            if mod_sig.ndim == 3:
                assert mod_sig.size(1) in (1, n_ch)
            mr = _channel_rows_of(x, mod_sig)[1]                      # a mod_sig without a channel axis: shared by the channels
        elif mod_sig is not None:
            n_mod = (W + 3) // 4
            assert mod_sig.size(0) == bs and mod_sig.ndim in (2, 3)
            if mod_sig.ndim == 3:
                assert mod_sig.size(1) in (1, n_ch)
            if mod_sig.size(-1) != n_mod:
                assert mod_sig.size(-1) == W, "mod_sig: one value per 4 samples or full rate"
                mod_sig = mod_sig[..., ::4]                           # samples 0, 4, 8, ...: a slice autograd handles
            if mod_sig.ndim == 2 or mod_sig.size(1) == 1:
                mod_sig = mod_sig.reshape(bs, 1, n_mod).expand(-1, n_ch, -1)
            mr = mod_sig.reshape(rows, n_mod).float().contiguous()
        ps = (None if rate_hz is None else vec(rate_hz), vec(depth), vec(centre_frequency_hz), vec(feedback), vec(mix))
        return xr, mr, ps, lead_rows, n, (bs, n_ch)

    def apply_effect(self, x: T, mod_sig: Optional[T] = None, rate_hz: Optional[Param] = None, depth: Param = 1.0,
                     centre_frequency_hz: Param = 1300.0, feedback: Param = 0.0, mix: Param = 1.0, lead=None,
                     mod_sig_low_rate: bool = False) -> T:
        params = (depth, centre_frequency_hz, feedback, mix)
        if not (torch.is_grad_enabled() and (x.requires_grad or (mod_sig is not None and mod_sig.requires_grad) or
                                             any(isinstance(p, T) and p.requires_grad for p in params))):
            if isinstance(rate_hz, T) and rate_hz.requires_grad and torch.is_grad_enabled():
                raise ValueError("PhaserModule has no gradient with respect to rate_hz: pass the LFO as mod_sig instead")
            return self.forward(x, mod_sig, rate_hz, depth, centre_frequency_hz, feedback, mix, lead, mod_sig_low_rate)
        xr, mr, ps, lead_rows, n, (bs, n_ch) = self._prepare(x, mod_sig, rate_hz, *params, lead, mod_sig_low_rate)
        if mod_sig_low_rate:
            y = _PhaserLowRateFunction.apply(xr, mr, *ps[1:], lead_rows, n_ch, self.sr, n)
        else:
            y = _PhaserFunction.apply(xr, mr, *ps, lead_rows, n_ch, self.sr, n)
        return y.view(bs, n_ch, n)

    def forward(self, x: T, mod_sig: Optional[T] = None, rate_hz: Optional[Param] = None, depth: Param = 1.0,
                centre_frequency_hz: Param = 1300.0, feedback: Param = 0.0, mix: Param = 1.0, lead=None,
                mod_sig_low_rate: bool = False) -> T:
        with torch.no_grad():
            xr, mr, ps, lead_rows, n, (bs, n_ch) = self._prepare(x, mod_sig, rate_hz, depth, centre_frequency_hz, feedback,
                                                                 mix, lead, mod_sig_low_rate)
            p = {k: _per_row(v.float(), n_ch) for k, v in zip(("rate_hz", "depth", "centre_frequency_hz", "feedback", "mix"), ps)
                 if v is not None}
            if mr is None:
                y = phaser_forward(xr, p, lead_rows, self.sr, n)
            elif mod_sig_low_rate:
                y = phaser_forward_stash_lr(xr, p, lead_rows, self.sr, n, mr)[0]
            else:
                y, _ = phaser_forward_stash(xr, p, lead_rows, self.sr, n, mod=mr)
        return y.view(bs, n_ch, n)


class _TremoloFunction(torch.autograd.Function):
    """y = tremolo(x, mod, mix) over (clip, channel) rows; the (bs,) mix is shared by a clip's n_ch rows, so its gradient
    is summed over the channels (in fp64) before it is rounded to fp32.  one_minus_mix gets no gradient of its own: d mix
    includes that path."""

    @staticmethod
    def forward(ctx, x, mod_sig, mix, one_minus_mix, n_ch):
        consts = {"mix": _per_row(mix.detach(), n_ch), "one_minus_mix": _per_row(one_minus_mix.detach(), n_ch)}
        y = tremolo_forward(x.detach(), mod_sig.detach(), consts)
        ctx.save_for_backward(x, mod_sig)
        ctx.consts, ctx.n_ch = consts, n_ch
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, mod_sig = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx, dmod, dmix = tremolo_backward(dy, x, mod_sig, ctx.consts, need_dx=need[0], need_dmod=need[1], need_dmix=need[2])
        if dmix is not None:
            dmix = dmix.view(-1, ctx.n_ch).sum(1).float()
        return dx, dmod, dmix, None, None


class TremoloModule(nn.Module):
    """The tremolo of fx.py:13-22 (``apply_tremolo``) as a module in the shape of ``PhaserModule``, on the
    ``mx_tremolo_fwd`` / ``mx_tremolo_bwd`` kernels.

    x (bs, n_ch, N): the channels are rows that share their clip's LFO and mix.  mod_sig (bs, n_mod) or
    (bs, 1 | n_ch, n_mod) at any 1 <= n_mod <= N: a row shorter than N is resampled in-kernel exactly as
    ``util.linear_interpolate_last_dim(mod_sig, N, align_corners=True)`` would, and its gradient has mod_sig's own shape.
    mix: a python float or a (bs,) tensor in [0, 1] -- one value PER CLIP, which the reference's scalar assert (fx.py:21)
    does not allow; a float or a one-element tensor reproduces ``apply_tremolo`` bit for bit.

    ``forward`` runs under no_grad.  ``apply_effect`` carries a grad_fn when grad mode is on and x, mod_sig or a tensor mix
    requires grad; the gradients of mod_sig and mix are summed over a clip's channels.  A python-float mix gets no
    gradient.  The effect has no state, so there is no stash: the backward recomputes the LFO values."""

    def _prepare(self, x: T, mod_sig: T, mix: Param):
        assert x.ndim == 3
        bs, n_ch, n = x.shape
        assert mod_sig.size(0) == bs and mod_sig.ndim in (2, 3) and 1 <= mod_sig.size(-1) <= n
        if mod_sig.ndim == 3:
            assert mod_sig.size(1) in (1, n_ch)
        consts = derive_tremolo_constants(bs, x.device, mix)
        xr, mr = _channel_rows_of(x, mod_sig)
        return xr, mr, consts, (bs, n_ch, n)

    def apply_effect(self, x: T, mod_sig: T, mix: Param = 1.0) -> T:
        if not (torch.is_grad_enabled() and (x.requires_grad or mod_sig.requires_grad or
                                             (isinstance(mix, T) and mix.requires_grad))):
            return self.forward(x, mod_sig, mix)
        xr, mr, consts, shape = self._prepare(x, mod_sig, mix)
        return _TremoloFunction.apply(xr, mr, consts["mix"], consts["one_minus_mix"], shape[1]).view(shape)

    def forward(self, x: T, mod_sig: T, mix: Param = 1.0) -> T:
        with torch.no_grad():
            xr, mr, consts, shape = self._prepare(x, mod_sig, mix)
            y = tremolo_forward(xr, mr, {k: _per_row(v, shape[1]) for k, v in consts.items()})
        return y.view(shape)


# ---- learned effect parameters (csrc/fx_params.hip, DESIGN K16) ------------------------------------------------------
FX_KINDS = ("flanger", "chorus", "phaser", "tremolo", "dry")       # the kind codes of the kernels' row_kind vector
FX_SLOTS = ("lfo_scale", "min_delay", "feedback", "depth", "mix", "centre_frequency_hz")   # rows of the (6, B) gradients
FX_CONSTS = ("lfo_scale", "min_delay", "feedback", "depth", "mix", "one_minus_mix", "centre_frequency_hz")
# the parameter names of every kind, in the canonical order of ``LearnedFxParams.names``, and the slot each one fills
FX_PARAM_NAMES = {"flanger": ("feedback", "min_delay_width", "width", "depth", "mix"),
                  "chorus": ("feedback", "min_delay_width", "width", "depth", "mix"),
                  "tremolo": ("mix",),
                  "phaser": ("depth", "centre_frequency_hz", "feedback", "mix")}
FX_NAME_SLOT = {"width": "lfo_scale", "min_delay_width": "min_delay", "feedback": "feedback", "depth": "depth", "mix": "mix",
                "centre_frequency_hz": "centre_frequency_hz"}
FX_MAX_LEARNED = 16                                                 # FXP_MAX_ENTRIES of csrc/fx_params_common.h


def _fx_param_range(kind: str, name: str) -> Tuple[float, float, bool, bool]:
    """(lo, hi, lo_open, hi_open): what ``_check_param`` / ``derive_phaser_params(check=True)`` accept for a parameter."""
    if name == "centre_frequency_hz":
        return 0.0, float("inf"), True, False
    if name == "feedback":
        return (-1.0, 1.0, True, True) if kind == "phaser" else (0.0, 1.0, False, True)
    return 0.0, 1.0, False, False


def fx_params_expand(raw: T, tab_f: T, tab_i: T, raw_gain: float, row_kind: T, max_lfo_delay: Optional[T],
                     max_min_delay: Optional[T], consts: Dict[str, T], values: Optional[T] = None) -> T:
    """Launch mx_fx_params_expand: the P mapped values of ``raw`` (P,) fp32 written into the rows of their kind of the (B,)
    fp32 vectors of ``consts`` (keys out of ``FX_CONSTS``; a missing key skips its slot), in place; rows and slots without
    an entry keep what they hold.  tab_f (2, P) fp64 and tab_i (3, P) int32 as ``LearnedFxParams`` builds them; row_kind (B,)
    int32 (``FX_KINDS`` codes).  Returns values (P,) fp32."""
    P, B = raw.numel(), row_kind.numel()
    assert raw.dtype == torch.float32 and tab_f.shape == (2, P) and tab_f.dtype == torch.float64
    assert tab_i.shape == (3, P) and tab_i.dtype == torch.int32 and row_kind.dtype == torch.int32
    for k, v in consts.items():
        assert k in FX_CONSTS and v.shape == (B,) and v.dtype == torch.float32, k
    for v in (max_lfo_delay, max_min_delay):
        assert v is None or (v.shape == (B,) and v.dtype == torch.float32)
    if values is None:
        values = torch.empty((P,), device=raw.device, dtype=torch.float32)
    assert values.shape == (P,) and values.dtype == torch.float32
    _hip.call("mx_fx_params_expand", _hip.ptr(raw), _hip.ptr(tab_f), _hip.ptr(tab_i), P, float(raw_gain), _hip.ptr(row_kind),
              _hip.ptr(max_lfo_delay), _hip.ptr(max_min_delay), B, *[_hip.ptr(consts.get(k)) for k in FX_CONSTS],
              _hip.ptr(values), _hip.stream())
    return values


def fx_params_grad(grads: T, raw: T, tab_f: T, tab_i: T, raw_gain: float, row_kind: T, max_lfo_delay: T, max_min_delay: T,
                   scale: float = 1.0) -> T:
    """Launch mx_fx_params_grad: scale * d loss / d raw (P,) fp32 from grads (6, B) fp64, the per-clip gradients of the
    constants in ``FX_SLOTS`` order as the effect adjoints write them (rows of kinds without an entry for a slot are not
    read and may be uninitialised).  Deterministic."""
    P, B = raw.numel(), row_kind.numel()
    assert grads.shape == (len(FX_SLOTS), B) and grads.dtype == torch.float64
    assert raw.dtype == torch.float32 and tab_f.shape == (2, P) and tab_i.shape == (3, P)
    assert max_lfo_delay.shape == max_min_delay.shape == (B,) and max_lfo_delay.dtype == max_min_delay.dtype == torch.float32
    d_raw = torch.empty((P,), device=raw.device, dtype=torch.float32)
    _hip.call("mx_fx_params_grad", _hip.ptr(grads), _hip.ptr(raw), _hip.ptr(tab_f), _hip.ptr(tab_i), P, float(raw_gain),
              _hip.ptr(row_kind), _hip.ptr(max_lfo_delay), _hip.ptr(max_min_delay), B, float(scale), _hip.ptr(d_raw),
              _hip.stream())
    return d_raw


class _FxParamTable(nn.Module):
    """What ``LearnedFxParams`` and ``FxParamHead`` share: the ``spec`` grammar and its checks, ``names`` / ``kinds`` / ``fixed``
    and the kernels' table.  ``_parse`` returns raw's initial values, logit(init) / raw_gain per entry; ``what`` names the
    argument in the error messages."""

    def _parse(self, spec: Dict[str, Dict[str, object]], raw_gain: float, what: str) -> T:
        import math
        if not isinstance(spec, dict) or not spec:
            raise ValueError(f"{what}: a dict keyed by effect kind")
        if not (isinstance(raw_gain, (int, float)) and math.isfinite(raw_gain) and raw_gain > 0):
            raise ValueError(f"raw_gain {raw_gain!r}: a positive number")
        self.raw_gain = float(raw_gain)
        self.names, self.fixed = [], {}
        lo, hi, is_log, slot, kind_code, init_raw = [], [], [], [], [], []
        for kind, params in spec.items():
            if kind not in FX_PARAM_NAMES:
                raise ValueError(f"{what}: unknown kind '{kind}' (supported: {tuple(FX_PARAM_NAMES)})")
            if not isinstance(params, dict):
                raise ValueError(f"{what}.{kind}: a dict of parameter names")
            for name in params:
                if name not in FX_PARAM_NAMES[kind]:
                    raise ValueError(f"{what}: '{kind}' has no parameter '{name}' (it has {FX_PARAM_NAMES[kind]})")
            for name in FX_PARAM_NAMES[kind]:
                if name not in params:
                    continue
                entry, full = params[name], f"{kind}.{name}"
                a, b, a_open, b_open = _fx_param_range(kind, name)
                if not isinstance(entry, dict):
                    v = float(entry)
                    if not ((v > a if a_open else v >= a) and (v < b if b_open else v <= b)):
                        raise ValueError(f"{what}.{full} = {v}: outside the effect's range")
                    self.fixed[(kind, name)] = v
                    continue
                unknown = set(entry) - {"min", "max", "init", "scale"}
                if unknown or not {"min", "max", "init"} <= set(entry):
                    raise ValueError(f"{what}.{full}: keys min, max, init and optionally scale (got {sorted(entry)})")
                mn, mx, init = float(entry["min"]), float(entry["max"]), float(entry["init"])
                scale = entry.get("scale", "log" if name == "centre_frequency_hz" else "lin")
                if scale not in ("lin", "log"):
                    raise ValueError(f"{what}.{full}: scale '{scale}' (lin or log)")
                if not all(math.isfinite(v) for v in (mn, mx, init)) or not mn < init < mx:
                    raise ValueError(f"{what}.{full}: min < init < max does not hold ({mn}, {init}, {mx})")
                if not ((mn > a if a_open else mn >= a) and (mx < b if b_open else mx <= b)):
                    raise ValueError(f"{what}.{full}: the range [{mn}, {mx}] must lie inside "
                                     f"{'(' if a_open else '['}{a}, {b}{')' if b_open else ']'}")
                if scale == "log" and mn <= 0:
                    raise ValueError(f"{what}.{full}: a log scale needs min > 0")
                s = (math.log(init / mn) / math.log(mx / mn)) if scale == "log" else (init - mn) / (mx - mn)
                self.names.append(full)
                lo.append(mn), hi.append(mx), is_log.append(int(scale == "log"))
                slot.append(FX_SLOTS.index(FX_NAME_SLOT[name])), kind_code.append(FX_KINDS.index(kind))
                init_raw.append(math.log(s / (1.0 - s)) / self.raw_gain)
        if not 1 <= len(self.names) <= FX_MAX_LEARNED:
            raise ValueError(f"{what}: {len(self.names)} learned entries (1 .. {FX_MAX_LEARNED} are supported)")
        self.kinds = tuple(spec)
        # the kernels' table; not part of the state dict (the spec rebuilds it)
        self.register_buffer("tab_f", torch.tensor([lo, hi], dtype=torch.float64), persistent=False)
        self.register_buffer("tab_i", torch.tensor([is_log, slot, kind_code], dtype=torch.int32), persistent=False)
        return torch.tensor(init_raw, dtype=torch.float64).float()

    def learned(self, kind: str) -> Tuple[str, ...]:
        """The learned parameter names of a kind."""
        return tuple(n.split(".", 1)[1] for n in self.names if n.split(".", 1)[0] == kind)

    def covers(self, kind: str, name: str) -> bool:
        return (kind, name) in self.fixed or f"{kind}.{name}" in self.names

    def _map(self, raw: T) -> T:
        """The mapped values of raw (..., P), fp64, by torch expressions."""
        s = torch.sigmoid(self.raw_gain * raw.double())
        lo, hi = self.tab_f[0], self.tab_f[1]
        log = self.tab_i[0] != 0
        lo_l, hi_l = torch.where(log, lo, torch.ones_like(lo)).log(), torch.where(log, hi, torch.ones_like(hi)).log()
        return torch.where(log, torch.exp(lo_l + (hi_l - lo_l) * s), lo + (hi - lo) * s)


class LearnedFxParams(_FxParamTable):
    """Effect parameters fitted together with the LFO extractor (``lightning.LFOExtractionThroughEffect(learned_fx=...)``):
    ONE shared value per (kind, name), not one per clip.  ``spec``: a dict keyed by kind (``flanger``, ``chorus``,
    ``tremolo``, ``phaser``); under each kind a parameter name maps to ``{min, max, init[, scale: lin | log]}`` = learned, or
    to a bare number = fixed (not learned, but it overrides the batch's value on the rows of that kind).

    One parameter ``raw`` (P,) fp32, 1 <= P <= 16; ``names`` lists its entries as ``"flanger.feedback"``: the kinds in spec
    order, under each kind the names in the order of ``FX_PARAM_NAMES``.  value = min + (max - min) sigmoid(raw_gain raw); with
    ``scale: log`` (the default of ``centre_frequency_hz``) the same map between log min and log max.  raw starts at
    logit(init) / raw_gain.  ``raw_gain``: Adam's step does not depend on the gradient's scale, so a gain k makes the step in
    the mapped domain k times longer at the learning rate the fitted scalars share with the network.

    Every learned range lies inside what the effect accepts, ends included where a value rounded onto an end is still legal:
    feedback of the flanger / chorus max < 1, of the phaser -1 < min and max < 1, centre_frequency_hz min > 0.  ValueError
    for anything else: unknown kinds or names, min < init < max violated, a log scale with min <= 0, no or more than 16
    learned entries.

    ``values()``: the P mapped values in fp64 by torch (any device).  The step's path is ``expand`` / ``grad``: the
    ``mx_fx_params_expand`` / ``mx_fx_params_grad`` launches."""

    def __init__(self, spec: Dict[str, Dict[str, object]], raw_gain: float = 1.0) -> None:
        super().__init__()
        self.raw = nn.Parameter(self._parse(spec, raw_gain, "learned_fx"))

    def values(self) -> T:
        """The P mapped values, fp64, by torch expressions (differentiable with respect to ``raw``)."""
        return self._map(self.raw)

    def expand(self, consts: Dict[str, T], row_kind: T, max_lfo_delay: Optional[T], max_min_delay: Optional[T]) -> T:
        """``fx_params_expand`` with this module's table: writes into ``consts`` in place, returns values (P,) fp32."""
        return fx_params_expand(self.raw.detach(), self.tab_f, self.tab_i, self.raw_gain, row_kind, max_lfo_delay,
                                max_min_delay, consts)

    def grad(self, grads: T, row_kind: T, max_lfo_delay: T, max_min_delay: T, scale: float = 1.0) -> T:
        """``fx_params_grad`` with this module's table: d loss / d raw (P,) fp32."""
        return fx_params_grad(grads, self.raw.detach(), self.tab_f, self.tab_i, self.raw_gain, row_kind, max_lfo_delay,
                              max_min_delay, scale)


# ---- per-clip effect parameters from a head on the extractor's latent (csrc/fx_head.hip, DESIGN K17) -------------------------
FX_HEAD_MAX_CHANNELS = 1024                                         # FXH_MAX_C of csrc/fx_head.hip


def fx_head_forward(latent: T, weight: T, bias: T, tab_f: T, tab_i: T, raw_gain: float, row_kind: T,
                    max_lfo_delay: Optional[T], max_min_delay: Optional[T], consts: Dict[str, T],
                    pooled: Optional[T] = None, raw_rows: Optional[T] = None,
                    values: Optional[T] = None) -> Tuple[T, T, T]:
    """Launch mx_fx_head_fwd: latent (B, C, W) fp32 dense -> pooled (B, C) = its mean over w, raw_rows (B, P) = bias + pooled
    weight^T, values (B, P) = the map of ``fx_params_expand`` applied to raw_rows, all fp32; on the rows of an entry's kind the
    value is also written into the (B,) fp32 vectors of ``consts`` (keys out of ``FX_CONSTS``; a missing key skips its slot),
    in place, by the rule of ``fx_params_expand``; rows and slots without an entry keep what they hold.  weight (P, C), bias
    (P,) fp32; the table and row_kind as there.  Returns (pooled, raw_rows, values)."""
    assert latent.ndim == 3 and latent.dtype == torch.float32
    B, C, W = latent.shape
    P = bias.numel()
    assert weight.shape == (P, C) and weight.dtype == bias.dtype == torch.float32 and bias.shape == (P,)
    assert tab_f.shape == (2, P) and tab_f.dtype == torch.float64 and tab_i.shape == (3, P) and tab_i.dtype == torch.int32
    assert row_kind.shape == (B,) and row_kind.dtype == torch.int32
    for k, v in consts.items():
        assert k in FX_CONSTS and v.shape == (B,) and v.dtype == torch.float32, k
    for v in (max_lfo_delay, max_min_delay):
        assert v is None or (v.shape == (B,) and v.dtype == torch.float32)
    dev = latent.device
    pooled = torch.empty((B, C), device=dev, dtype=torch.float32) if pooled is None else pooled
    raw_rows = torch.empty((B, P), device=dev, dtype=torch.float32) if raw_rows is None else raw_rows
    values = torch.empty((B, P), device=dev, dtype=torch.float32) if values is None else values
    assert pooled.shape == (B, C) and raw_rows.shape == values.shape == (B, P)
    assert pooled.dtype == raw_rows.dtype == values.dtype == torch.float32
    _hip.call("mx_fx_head_fwd", _hip.ptr(latent), B, C, W, _hip.ptr(weight), _hip.ptr(bias), _hip.ptr(tab_f), _hip.ptr(tab_i), P,
              float(raw_gain), _hip.ptr(row_kind), _hip.ptr(max_lfo_delay), _hip.ptr(max_min_delay),
              *[_hip.ptr(consts.get(k)) for k in FX_CONSTS], _hip.ptr(pooled), _hip.ptr(raw_rows), _hip.ptr(values),
              _hip.stream())
    return pooled, raw_rows, values


def fx_head_backward(grads: T, raw_rows: T, pooled: T, weight: T, tab_f: T, tab_i: T, raw_gain: float, row_kind: T,
                     max_lfo_delay: T, max_min_delay: T, W: int, scale: float = 1.0, need_d_raw_rows: bool = False,
                     need_d_latent: bool = True) -> Tuple[Optional[T], T, T, Optional[T]]:
    """Launch mx_fx_head_bwd: from grads (6, B) fp64 (the per-clip gradients of the constants in ``FX_SLOTS`` order, as the
    effect adjoints write them; rows of kinds without an entry for a slot are not read) and what ``fx_head_forward`` returned,
    (d_raw_rows (B, P) or None, d_bias (P,), d_weight (P, C), d_latent (B, C, W) or None), all fp32, times ``scale``.  Every
    element of d_latent is written (rows without an entry: zeros).  Deterministic."""
    B, P = raw_rows.shape
    C = pooled.size(1)
    assert grads.shape == (len(FX_SLOTS), B) and grads.dtype == torch.float64
    assert raw_rows.dtype == pooled.dtype == weight.dtype == torch.float32 and pooled.shape == (B, C) and weight.shape == (P, C)
    assert tab_f.shape == (2, P) and tab_f.dtype == torch.float64 and tab_i.shape == (3, P) and tab_i.dtype == torch.int32
    assert row_kind.shape == (B,) and row_kind.dtype == torch.int32 and W >= 1
    assert max_lfo_delay.shape == max_min_delay.shape == (B,) and max_lfo_delay.dtype == max_min_delay.dtype == torch.float32
    dev = raw_rows.device
    d_rows = torch.empty((B, P), device=dev, dtype=torch.float32) if need_d_raw_rows else None
    d_bias = torch.empty((P,), device=dev, dtype=torch.float32)
    d_weight = torch.empty((P, C), device=dev, dtype=torch.float32)
    d_latent = torch.empty((B, C, W), device=dev, dtype=torch.float32) if need_d_latent else None
    _hip.call("mx_fx_head_bwd", _hip.ptr(grads), _hip.ptr(raw_rows), _hip.ptr(pooled), _hip.ptr(weight), _hip.ptr(tab_f),
              _hip.ptr(tab_i), P, float(raw_gain), _hip.ptr(row_kind), _hip.ptr(max_lfo_delay), _hip.ptr(max_min_delay), B, C,
              int(W), float(scale), _hip.ptr(d_rows), _hip.ptr(d_bias), _hip.ptr(d_weight), _hip.ptr(d_latent), _hip.stream())
    return d_rows, d_bias, d_weight, d_latent


class FxParamHead(_FxParamTable):
    """Effect parameters PER CLIP, predicted from the extractor's latent (``lightning.LFOExtractionThroughEffect(fx_head=...)``):
    raw[b] = bias + weight mean_w latent[b, :, w], then the map of ``LearnedFxParams`` entry by entry.  ``spec``, its checks
    and ValueErrors, ``names``, ``kinds``, ``fixed``, ``learned``, ``covers``, ``raw_gain`` and the table are those of
    ``LearnedFxParams``; a bare number fixes a parameter for every clip.

    Parameters ``weight`` (P, in_ch) fp32, zeros, and ``bias`` (P,) fp32 = logit(init) / raw_gain: a fresh head predicts
    ``init`` for every clip, with the very bits ``LearnedFxParams`` writes, and departs from it only as ``weight`` learns.
    in_ch: the latent's channel count, 1 .. 1024 (64 for ``models.Spectral2DCNN``).

    ``values(latent)``: the (B, P) mapped values in fp64 by torch expressions (any device, differentiable).  The step's path
    is ``forward_rows`` / ``backward_rows``: the ``mx_fx_head_fwd`` / ``mx_fx_head_bwd`` launches."""

    def __init__(self, spec: Dict[str, Dict[str, object]], in_ch: int = 64, raw_gain: float = 1.0) -> None:
        super().__init__()
        if not (isinstance(in_ch, int) and 1 <= in_ch <= FX_HEAD_MAX_CHANNELS):
            raise ValueError(f"in_ch {in_ch!r}: 1 .. {FX_HEAD_MAX_CHANNELS} latent channels")
        self.in_ch = in_ch
        bias = self._parse(spec, raw_gain, "fx_head")
        self.weight = nn.Parameter(torch.zeros((bias.numel(), in_ch), dtype=torch.float32))
        self.bias = nn.Parameter(bias)

    def values(self, latent: T) -> T:
        """The (B, P) mapped values of latent (B, in_ch, W), fp64, by torch expressions."""
        assert latent.ndim == 3 and latent.size(1) == self.in_ch
        pooled = latent.double().mean(-1)
        return self._map(self.bias.double() + pooled @ self.weight.double().t())

    def forward_rows(self, latent: T, consts: Dict[str, T], row_kind: T, max_lfo_delay: Optional[T],
                     max_min_delay: Optional[T]) -> Tuple[T, T, T]:
        """``fx_head_forward`` with this module's parameters and table: writes into ``consts`` in place, returns (pooled,
        raw_rows, values)."""
        return fx_head_forward(latent, self.weight.detach(), self.bias.detach(), self.tab_f, self.tab_i, self.raw_gain,
                               row_kind, max_lfo_delay, max_min_delay, consts)

    def backward_rows(self, grads: T, raw_rows: T, pooled: T, row_kind: T, max_lfo_delay: T, max_min_delay: T, W: int,
                      scale: float = 1.0, need_d_latent: bool = True) -> Tuple[T, T, Optional[T]]:
        """``fx_head_backward`` with this module's weight and table: (d_bias (P,), d_weight (P, in_ch), d_latent (B, in_ch,
        W) or None)."""
        return fx_head_backward(grads, raw_rows, pooled, self.weight.detach(), self.tab_f, self.tab_i, self.raw_gain, row_kind,
                                max_lfo_delay, max_min_delay, W, scale, need_d_latent=need_d_latent)[1:]

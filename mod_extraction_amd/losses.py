"""Host mirror of mod_extraction/losses.py.

``get_loss_func_by_name`` (losses.py:142-160) returns ``nn.Module``s with the reference's names and
call signature; l1 / fdl1 / sdl1 / mse -- the LFO-extraction losses -- are evaluated by the fused
``mx_lfo_loss`` HIP kernel (all four terms and d/d(y_hat) in one launch).  ``lfo_loss`` is the fused
weighted form that ``lightning.LFOExtraction`` uses (lightning.py:33-62).
"""
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor as T, nn

from . import _hip
from .mrstft import RUN_MIN, ola_scratch_floats, run_geometry

_LFO_TERMS = ("l1", "fdl1", "sdl1", "mse")


class _LFOLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y_hat: T, y: T, w_l1: float, w_fd: float, w_sd: float, w_mse: float):
        assert y_hat.shape == y.shape
        n = y_hat.size(-1)
        yh = y_hat.reshape(-1, n).contiguous().float()
        yt = y.reshape(-1, n).contiguous().float()
        B = yh.size(0)
        part = torch.empty((B, 4), device=yh.device, dtype=torch.float32)
        losses = torch.empty(5, device=yh.device, dtype=torch.float32)
        grad = torch.empty_like(yh)
        _hip.call("mx_lfo_loss", _hip.ptr(yh), _hip.ptr(yt), B, n, float(w_l1), float(w_fd), float(w_sd),
                  float(w_mse), _hip.ptr(part), _hip.ptr(losses), _hip.ptr(grad), _hip.stream())
        ctx.save_for_backward(grad)
        ctx.shape = y_hat.shape
        return losses

    @staticmethod
    def backward(ctx, g: T):
        (grad,) = ctx.saved_tensors
        return (grad * g[4]).view(ctx.shape), None, None, None, None, None


def lfo_loss(y_hat: T, y: T, weights: Dict[str, float]) -> Tuple[T, Dict[str, T]]:
    """Weighted LFO loss: returns (total, {name: term}); only weights > 0 enter the total
    (lightning.py:48-52) but every named term is reported."""
    for k in weights:
        if k not in _LFO_TERMS:
            raise KeyError(k)
    # losses.py:12 (central_diff asserts more than 2 points): the reference raises for rows too short to differentiate
    n = y_hat.size(-1)
    assert "fdl1" not in weights or n > 2, "fdl1: central difference needs more than 2 points"
    assert "sdl1" not in weights or n > 4, "sdl1: second central difference needs more than 4 points"
    w = [float(weights.get(k, 0.0)) for k in _LFO_TERMS]
    losses = _LFOLossFn.apply(y_hat, y, *w)
    return losses[4], {k: losses[i].detach() for i, k in enumerate(_LFO_TERMS) if k in weights}


class _SingleTerm(nn.Module):
    term = "l1"

    def forward(self, input: T, target: T) -> T:
        return lfo_loss(input, target, {self.term: 1.0})[0]


class L1Loss(_SingleTerm):
    term = "l1"


class FirstDerivativeL1Loss(_SingleTerm):
    term = "fdl1"

    @staticmethod
    def calc_first_derivative(x: T) -> T:
        """losses.py:80-84 (analysis helper; the loss itself differentiates inside the kernel)."""
        assert x.size(-1) > 2
        return (x[..., 2:] - x[..., :-2]) / 2.0


class SecondDerivativeL1Loss(_SingleTerm):
    term = "sdl1"

    @staticmethod
    def calc_second_derivative(x: T) -> T:
        """losses.py:97-102."""
        return FirstDerivativeL1Loss.calc_first_derivative(FirstDerivativeL1Loss.calc_first_derivative(x))


class MSELoss(_SingleTerm):
    term = "mse"


def logmel_scratch_floats(B: int, Tn: int, n_fft: int, hop: int) -> int:
    """Workspace floats of ``mx_logmel_l1_loss`` for the gradient (include/modex_hip.h): per clip frames * hop run sums plus
    one tail of n_fft - hop positions per run of F frames."""
    return ola_scratch_floats(1, B, Tn, n_fft, hop)


def logmel_l1_value_and_grad(mod: "LogMelLoss", a: T, t: T, need_grad: bool = True, scale: float = 1.0,
                             dx: Optional[T] = None, accumulate: bool = False) -> Tuple[T, Optional[T]]:
    """a (prediction), t (target): (rows, T) with unit inner stride.  Returns (scale * loss as a device scalar,
    d (scale * loss) / d a or None) from ONE ``mx_logmel_l1_loss`` call.  ``dx``: a (rows, T) float32 tensor with unit inner
    stride to write the gradient into (``accumulate``: add it onto what ``dx`` holds) instead of a fresh one."""
    assert a.shape == t.shape and a.ndim == 2 and a.stride(1) == 1 and t.stride(1) == 1
    assert a.dtype == torch.float32 and t.dtype == torch.float32
    B, Tn = a.shape
    sp = mod.spectrogram
    n_fft, hop = sp.n_fft, sp.hop_length
    if Tn <= n_fft // 2:
        raise ValueError(f"log_mel_l1: reflect padding needs more than n_fft/2 = {n_fft // 2} samples, got {Tn}")
    dev = a.device
    if sp.mel_scale.fb.device != dev:
        sp.to(dev)
    # one partial per workgroup, a workgroup takes at least one run: at most ceil(frames / RUN_MIN) per clip
    part = torch.empty(B * -(-run_geometry(Tn, n_fft, hop)[0] // RUN_MIN), device=dev, dtype=torch.float64)
    value = torch.empty((), device=dev, dtype=torch.float32)
    if need_grad:
        if dx is None:
            dx = torch.empty((B, Tn), device=dev, dtype=torch.float32)
            accumulate = False
        assert dx.shape == (B, Tn) and dx.stride(1) == 1 and dx.dtype == torch.float32
        scratch = torch.empty(logmel_scratch_floats(B, Tn, n_fft, hop), device=dev, dtype=torch.float32)
    else:
        dx, scratch = None, None
    lo, hi = sp.bands()
    _hip.call("mx_logmel_l1_loss", a.data_ptr(), a.stride(0), t.data_ptr(), t.stride(0), B, Tn,
              _hip.ptr(sp.spectrogram.window), _hip.ptr(sp.twiddle), _hip.ptr(sp.mel_scale.fb), _hip.ptr(lo), _hip.ptr(hi),
              n_fft, hop, sp.n_mels, float(mod.eps), float(scale), int(bool(accumulate)), _hip.ptr(part), _hip.ptr(scratch),
              _hip.ptr(value), None if dx is None else dx.data_ptr(), 0 if dx is None else dx.stride(0), _hip.stream())
    return value, dx


class LogMelLoss(nn.Module):
    """losses.py:105-130 (``log_mel_l1``): L1 between the log-mel spectrograms of input and target, evaluated by
    ``mx_logmel_l1_loss`` in value-only mode (any clip length above n_fft/2; no spectrogram is materialised).  The
    gradient reaches training through ``effect_losses.effect_loss_grad`` (``logmel_l1_value_and_grad``), not autograd:
    a prediction that requires grad raises instead of silently returning a constant."""

    def __init__(self, sr: float = 44100, n_fft: int = 1024, hop_len: int = 256, n_mels: int = 256,
                 eps: float = 1e-7) -> None:
        super().__init__()
        from .models import MelSpectrogramHIP
        self.eps, self.hop_len = eps, hop_len
        self.spectrogram = MelSpectrogramHIP(int(sr), n_fft, hop_len, n_mels)

    def forward(self, input: T, target: T) -> T:
        if input.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("log_mel_l1 is forward-only on this path (evaluation metric)")
        assert input.shape == target.shape and input.ndim == 3
        n = input.size(-1)
        a = input.detach().reshape(-1, n).contiguous().float()
        t = target.detach().reshape(-1, n).contiguous().float()
        return logmel_l1_value_and_grad(self, a, t, need_grad=False)[0]


def pre_emph_esr_value_and_grad(mod: "PreEmphESRLoss", a: T, t: T, need_grad: bool = True, scale: float = 1.0,
                                dx: Optional[T] = None, accumulate: bool = False,
                                need_value: bool = True) -> Tuple[Optional[T], Optional[T]]:
    """a (prediction), t (target): (rows, T) with unit inner stride.  Returns (scale * loss as a device scalar,
    d (scale * loss) / d a or None) from ONE launch: ``mx_pre_emph_esr_grad`` (value and gradient) or, without a gradient,
    ``mx_pre_emph_esr_sums``.  ``dx``: a (rows, T) float32 tensor with unit inner stride to write the gradient into
    (``accumulate``: add it onto what ``dx`` holds) instead of a fresh one.  ``need_value=False``: the value (a few small
    torch kernels on the per-clip sums) is not formed and None is returned in its place -- a TBPTT step that only
    back-propagates launches the gradient kernel alone."""
    assert a.shape == t.shape and a.ndim == 2 and a.stride(1) == 1 and t.stride(1) == 1
    assert a.dtype == torch.float32 and t.dtype == torch.float32
    if not a.is_cuda:
        raise _hip.HipLibraryError("mod_extraction_amd ops need tensors on a HIP device (no CPU fallback)")
    B, Tn = a.shape
    taps = mod.taps
    if taps.out_len(Tn) <= 0:
        raise ValueError(f"esr_pre with low_pass needs more than 1 sample, got {Tn}")
    part = torch.empty((B, 2), device=a.device, dtype=torch.float32)
    head = (a.data_ptr(), a.stride(0), t.data_ptr(), t.stride(0), B, Tn, _hip.ptr(taps.on(a.device)),
            len(taps.filter_cfs), int(taps.low_pass))
    if need_grad:
        if dx is None:
            dx = torch.empty((B, Tn), device=a.device, dtype=torch.float32)
            accumulate = False
        assert dx.shape == (B, Tn) and dx.stride(1) == 1 and dx.dtype == torch.float32
        _hip.call("mx_pre_emph_esr_grad", *head, float(scale), float(mod.eps), int(bool(accumulate)), _hip.ptr(part),
                  dx.data_ptr(), dx.stride(0), _hip.stream())
    else:
        dx = None
        _hip.call("mx_pre_emph_esr_sums", *head, _hip.ptr(part), _hip.stream())
    if not need_value:
        return None, dx
    value = (part[:, 0] / (part[:, 1] + mod.eps)).mean()                     # losses.py:34-38 on the filtered pair
    return (value if scale == 1.0 else scale * value), dx


class PreEmphESRLoss(nn.Module):
    """``esr_pre``: the reference's ``ESRLoss`` (losses.py:14-38: per-clip ratio, mean over the clips, eps 1e-8) applied to
    the outputs of ``WrightPreEmph(filter_cfs, low_pass)`` (wright_code.py:47-73), evaluated by ``mx_pre_emph_esr_sums``
    without materialising the filtered signals.  The module owns the tap buffer on the device.  Like ``LogMelLoss`` the
    gradient reaches training through ``effect_losses.effect_loss_grad`` (``pre_emph_esr_value_and_grad``), not autograd: a
    prediction that requires grad raises instead of silently returning a constant."""

    def __init__(self, filter_cfs=(-0.95, 1.0), low_pass: bool = False, eps: float = 1e-8) -> None:
        super().__init__()
        from .wright_code import PreEmphTaps
        self.taps = PreEmphTaps(filter_cfs, low_pass)
        self.eps = float(eps)

    def forward(self, input: T, target: T) -> T:
        if input.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("esr_pre is forward-only on this path (evaluation metric)")
        assert input.shape == target.shape and input.ndim == 3
        n = input.size(-1)
        a = input.detach().reshape(-1, n).contiguous().float()
        t = target.detach().reshape(-1, n).contiguous().float()
        return pre_emph_esr_value_and_grad(self, a, t, need_grad=False)[0]


def apply_reduction(losses: T, reduction: str = "none") -> T:
    """losses.py:133-139."""
    if reduction == "mean":
        return losses.mean()
    if reduction == "sum":
        return losses.sum()
    return losses


def get_loss_func_by_name(name: str) -> nn.Module:
    if name == "l1":
        return L1Loss()
    elif name == "fdl1":
        return FirstDerivativeL1Loss()
    elif name == "sdl1":
        return SecondDerivativeL1Loss()
    elif name == "mse":
        return MSELoss()
    elif name in ("esr", "dc"):
        from .effect_losses import get_effect_loss
        return get_effect_loss(name)
    elif name == "mrstft":
        from .effect_losses import get_effect_loss
        return get_effect_loss(name)
    elif name == "log_mel_l1":
        return LogMelLoss()
    elif name == "esr_pre":
        return PreEmphESRLoss()
    else:
        raise KeyError

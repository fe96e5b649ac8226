"""Host mirror of mod_extraction/wright_code.py (the CoreAudioML losses of Wright & Valimaki): the FIR pre-emphasis
``WrightPreEmph`` on the ``mx_pre_emph`` HIP kernel, and ``WrightESRLoss`` / ``WrightDCLoss`` (batch-global ratios,
``epsilon = 0.0``) from the per-row sums of ``mx_effect_loss_sums``.  Same names and call signatures as the reference:
the tensors are time-major ``(T, B, 1)`` and single-channel.
"""
from typing import Dict, Sequence, Tuple

import torch
from torch import Tensor as T, nn

from . import _hip

MAX_TAPS = 16           # PE_MAXK of csrc/pre_emph_loss.hip


class PreEmphTaps:
    """The pre-emphasis filter of a module: the taps as python floats, the low-pass flag, and ONE fp32 copy of the taps per
    device (uploaded on first use, so a module can be built without a device)."""

    def __init__(self, filter_cfs: Sequence[float], low_pass: bool = False) -> None:
        cfs = tuple(float(c) for c in filter_cfs)
        if not 1 <= len(cfs) <= MAX_TAPS:
            raise ValueError(f"filter_cfs: 1 .. {MAX_TAPS} taps are supported, got {len(cfs)}")
        self.filter_cfs, self.low_pass = cfs, bool(low_pass)
        self._on_device: Dict[torch.device, T] = {}

    def on(self, device: torch.device) -> T:
        taps = self._on_device.get(device)
        if taps is None:
            taps = self._on_device[device] = torch.tensor(self.filter_cfs, dtype=torch.float32, device=device)
        return taps

    def out_len(self, n: int) -> int:
        """Length of a filtered row of ``n`` samples (wright_code.py:69-71: the low-pass stage has no padding)."""
        return n - 1 if self.low_pass else n


def pre_emph_rows(taps: PreEmphTaps, x: T, transpose: bool = False, n: int = 0) -> T:
    """x (B, T) rows with unit inner stride -> F x (B, L); ``transpose``: x (B, L) -> F^T x (B, n) for rows of ``n``
    samples.  One ``mx_pre_emph`` launch."""
    assert x.ndim == 2 and (x.stride(1) == 1 or x.size(1) == 1) and x.dtype == torch.float32
    if not x.is_cuda:
        raise _hip.HipLibraryError("mod_extraction_amd ops need tensors on a HIP device (no CPU fallback)")
    B = x.size(0)
    if transpose:
        assert x.size(1) == taps.out_len(n)
    else:
        n = x.size(1)
    if taps.out_len(n) <= 0:
        raise ValueError(f"pre-emphasis with low_pass needs more than 1 sample, got {n}")
    out = torch.empty((B, n if transpose else taps.out_len(n)), device=x.device, dtype=torch.float32)
    # torch leaves the stride of a size-1 dimension arbitrary: a single row is given the stride of a packed one
    x_stride = x.stride(0) if B > 1 else x.size(1)
    _hip.call("mx_pre_emph", x.data_ptr(), x_stride, B, n, _hip.ptr(taps.on(x.device)), len(taps.filter_cfs),
              int(taps.low_pass), int(transpose), _hip.ptr(out), out.stride(0), _hip.stream())
    return out


class _PreEmphFn(torch.autograd.Function):
    """(T, B, 1) -> (L, B, 1) through ``mx_pre_emph``; the backward is the transposed filter (the same entry point with its
    transpose flag)."""

    @staticmethod
    def forward(ctx, x: T, taps: PreEmphTaps) -> T:
        assert x.ndim == 3 and x.size(2) == 1, "time-major single-channel (T, B, 1)"
        ctx.taps, ctx.n, ctx.dtype = taps, x.size(0), x.dtype
        rows = x.detach()[:, :, 0].t().contiguous().float()
        return pre_emph_rows(taps, rows).t().unsqueeze(-1).to(x.dtype)

    @staticmethod
    def backward(ctx, g: T):
        rows = g[:, :, 0].t().contiguous().float()
        return pre_emph_rows(ctx.taps, rows, transpose=True, n=ctx.n).t().unsqueeze(-1).to(ctx.dtype), None


class WrightPreEmph(nn.Module):
    """wright_code.py:47-73: FIR pre-emphasis with ``filter_cfs`` (zero history in front, same length), then with
    ``low_pass`` the taps [0.85, 1] without padding (one sample shorter).  Only supported for single-channel."""

    def __init__(self, filter_cfs: Sequence[float], low_pass: bool = False) -> None:
        super().__init__()
        self.taps = PreEmphTaps(filter_cfs, low_pass)
        self.low_pass = self.taps.low_pass
        self.zPad = len(self.taps.filter_cfs) - 1

    def forward(self, output: T, target: T) -> Tuple[T, T]:
        return _PreEmphFn.apply(output, self.taps), _PreEmphFn.apply(target, self.taps)


def _global_sums(output: T, target: T) -> Tuple[T, int]:
    """part (B, 4) of ``mx_effect_loss_sums`` for time-major (T, B, 1) tensors, and T."""
    if torch.is_grad_enabled() and output.requires_grad:
        raise NotImplementedError("WrightESRLoss / WrightDCLoss are forward-only (train with the esr_pre / dc gradient kernels)")
    assert output.shape == target.shape and output.ndim == 3 and output.size(2) == 1, "time-major single-channel (T, B, 1)"
    a = output.detach()[:, :, 0].t().contiguous().float()
    t = target.detach()[:, :, 0].t().contiguous().float()
    if not a.is_cuda:
        raise _hip.HipLibraryError("mod_extraction_amd ops need tensors on a HIP device (no CPU fallback)")
    B, n = a.shape
    part = torch.empty((B, 4), device=a.device, dtype=torch.float32)
    _hip.call("mx_effect_loss_sums", a.data_ptr(), a.stride(0), t.data_ptr(), t.stride(0), B, n, _hip.ptr(part),
              _hip.stream())
    return part, n


class WrightESRLoss(nn.Module):
    """wright_code.py:15-27: mean (target - output)^2 / (mean target^2 + epsilon) over the WHOLE batch -- one global ratio,
    unlike ``losses.ESRLoss``'s mean of per-clip ratios."""

    def __init__(self) -> None:
        super().__init__()
        self.epsilon = 0.0

    def forward(self, output: T, target: T) -> T:
        part, n = _global_sums(output, target)
        count = part.size(0) * n
        return (part[:, 1].sum() / count) / (part[:, 2].sum() / count + self.epsilon)


class WrightDCLoss(nn.Module):
    """wright_code.py:30-41: mean over clips of (time mean of target - time mean of output)^2, over the batch-global mean
    target^2 + epsilon."""

    def __init__(self) -> None:
        super().__init__()
        self.epsilon = 0.0

    def forward(self, output: T, target: T) -> T:
        part, n = _global_sums(output, target)
        count = part.size(0) * n
        return ((part[:, 3] / n) ** 2).mean() / (part[:, 2].sum() / count + self.epsilon)

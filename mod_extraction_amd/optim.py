"""AdamW on one flat fp32 buffer (K12, ``mx_adamw_step``), mirroring ``torch.optim.AdamW`` as the
reference configures it (configs/opt/adam_w.yml: lr 1e-4, betas (0.8, 0.99); torch defaults
eps 1e-8, weight_decay 0.01).

All trainable parameters of the module are re-homed as views into one contiguous buffer, and their
``.grad`` as views into a second one, so that a DDP step is ONE RCCL all-reduce over the flat
gradient followed by ONE kernel launch (the reference's Lightning/DDP path buckets per tensor).

Gradient clipping (the trainer keys ``gradient_clip_val`` / ``gradient_clip_algorithm`` of the reference's configs, i.e.
``clip_grad_norm_`` / ``clip_grad_value_``) belongs to this optimizer: with a clip set, the step is ``mx_grad_sumsq`` (norm
mode) + ``mx_adamw_step_clip`` and the clip coefficient never leaves the device; with the clip off the launches are exactly
``mx_adamw_step`` / ``mx_reduce_rows_adamw_step``.
"""
import contextlib
import math
from typing import Dict, Iterable, Iterator, List, Optional, Tuple

import torch
from torch import Tensor as T, nn

from . import _hip

SUMSQ_CHUNK = 4096              # elements one workgroup of mx_grad_sumsq sums per chunk (include/modex_hip.h)
SUMSQ_MAX_PARTIALS = 1024       # cap of its stage-1 grid; beyond it a workgroup takes further chunks
CLIP_MODES = {"norm": 1, "value": 2}


def sumsq_partials(n: int) -> int:
    """``G(n)`` of ``mx_grad_sumsq``: the number of fp64 partial sums its ``part`` workspace must hold."""
    assert n >= 1
    return min((int(n) + SUMSQ_CHUNK - 1) // SUMSQ_CHUNK, SUMSQ_MAX_PARTIALS)


def check_clip(val, algorithm) -> Tuple[Optional[float], str]:
    """Lightning's rule: ``None`` or a value ``<= 0`` switches clipping off; the algorithm is ``"norm"`` (default) or
    ``"value"``.  Returns ``(clip_val or None, algorithm)``."""
    algorithm = "norm" if algorithm is None else algorithm
    if algorithm not in CLIP_MODES:
        raise ValueError(f"gradient clip algorithm {algorithm!r}: expected 'norm' or 'value'")
    if val is None:
        return None, algorithm
    if isinstance(val, bool) or not isinstance(val, (int, float)) or not math.isfinite(val):
        raise ValueError(f"gradient clip value {val!r}: expected a finite number or None")
    return (float(val) if val > 0 else None), algorithm


class FlatAdamW:
    def __init__(self, params: Iterable[nn.Parameter], lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 0.01, clip_val: Optional[float] = None,
                 clip_algorithm: str = "norm") -> None:
        self.params: List[nn.Parameter] = [p for p in params if p.requires_grad]
        assert self.params, "no trainable parameters"
        dev = self.params[0].device
        assert all(p.device == dev and p.dtype == torch.float32 for p in self.params)
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), \
            float(weight_decay)
        n = sum(p.numel() for p in self.params)
        self.flat_param = torch.empty(n, device=dev, dtype=torch.float32)
        self.flat_grad = torch.zeros(n, device=dev, dtype=torch.float32)
        self.exp_avg = torch.zeros(n, device=dev, dtype=torch.float32)
        self.exp_avg_sq = torch.zeros(n, device=dev, dtype=torch.float32)
        self.step_count = 0
        off = 0
        for p in self.params:
            k = p.numel()
            self.flat_param[off:off + k].copy_(p.data.reshape(-1))
            p.data = self.flat_param[off:off + k].view(p.shape)
            p.grad = self.flat_grad[off:off + k].view(p.shape)
            off += k
        self.clip_val: Optional[float] = None
        self.clip_algorithm = "norm"
        self._clip_part: Optional[T] = None     # workspaces of mx_grad_sumsq / mx_adamw_step_clip, allocated once
        self._clip_stat: Optional[T] = None     # [sum of squares of flat_grad, the scale s the last clipped step applied]
        self._clip_grad_scale = 1.0
        self.set_gradient_clip(clip_val, clip_algorithm)

    def set_gradient_clip(self, val: Optional[float], algorithm: Optional[str] = "norm") -> None:
        """``val`` None or ``<= 0``: off.  ``algorithm`` "norm" (``clip_grad_norm_``, 2-norm over ALL parameters) or "value"
        (``clip_grad_value_``).  ``flat_grad`` itself is never clipped: the clip is applied as the step reads it."""
        self.clip_val, self.clip_algorithm = check_clip(val, algorithm)
        if self.clip_val is not None and self._clip_stat is None:
            dev = self.flat_param.device
            self._clip_part = torch.zeros(sumsq_partials(self.numel), device=dev, dtype=torch.float64)
            self._clip_stat = torch.zeros(2, device=dev, dtype=torch.float64)

    @property
    def last_grad_norm(self) -> Optional[T]:
        """2-norm of ``grad_scale * flat_grad`` as the last norm-clipped step saw it, before clipping (what
        ``clip_grad_norm_`` returns), as a 0-d fp64 DEVICE tensor -- formed on access from the device-resident sum of
        squares, so reading it costs no host round trip.  None with the clip off and in value mode."""
        if self._clip_stat is None or self.clip_val is None or self.clip_algorithm != "norm":
            return None
        return torch.sqrt(self._clip_stat[0]) * self._clip_grad_scale

    @property
    def last_clip_scale(self) -> Optional[T]:
        """The factor the last clipped step multiplied ``flat_grad`` by (``grad_scale`` times the clip coefficient; plain
        ``grad_scale`` in value mode), as a 0-d fp64 device tensor."""
        return None if self._clip_stat is None else self._clip_stat[1]

    @property
    def numel(self) -> int:
        return self.flat_param.numel()

    def zero_grad(self, set_to_none: bool = False) -> None:
        self.flat_grad.zero_()
        self.flat_grad._modex_fresh = False     # in-place gradient writes are armed only by direct_backward() below
        off = 0
        for p in self.params:          # re-attach views if something replaced .grad
            k = p.numel()
            if p.grad is None or p.grad.data_ptr() != self.flat_grad[off:off + k].data_ptr():
                p.grad = self.flat_grad[off:off + k].view(p.shape)
            off += k

    @contextlib.contextmanager
    def direct_backward(self) -> Iterator[None]:
        """Scope of ONE ``loss.backward()`` that may WRITE its parameter gradients into the flat buffer instead of
        accumulating (``models._direct_grad_views``).  The caller promises that the buffer holds nothing it wants to keep
        -- i.e. this is the first backward after ``zero_grad()`` -- and that neither ``torch.autograd.grad`` nor parameter
        hooks are used for that call (autograd is handed ``None`` for those inputs).  The flag is consumed by the first
        CNN backward inside the scope and is always cleared on exit, so a backward outside the scope (a weight penalty, a
        second sub-batch, a manual add into ``flat_grad``) takes the ordinary accumulate path."""
        self.flat_grad._modex_fresh = True
        try:
            yield
        finally:
            self.flat_grad._modex_fresh = False

    def _step_clip(self, grad_scale: float) -> None:
        mode = CLIP_MODES[self.clip_algorithm]
        self._clip_grad_scale = float(grad_scale)
        if mode == 1:
            _hip.call("mx_grad_sumsq", _hip.ptr(self.flat_grad), self.numel, _hip.ptr(self._clip_part), _hip.ptr(self._clip_stat),
                      _hip.stream())
        _hip.call("mx_adamw_step_clip", _hip.ptr(self.flat_param), _hip.ptr(self.flat_grad), _hip.ptr(self.exp_avg),
                  _hip.ptr(self.exp_avg_sq), self.numel, self.step_count, self.lr, self.betas[0], self.betas[1], self.eps,
                  self.weight_decay, float(grad_scale), mode, self.clip_val, _hip.ptr(self._clip_stat), _hip.stream())

    def step(self, grad_scale: float = 1.0) -> None:
        self.step_count += 1
        if self.clip_val is not None:
            return self._step_clip(grad_scale)
        _hip.call("mx_adamw_step", _hip.ptr(self.flat_param), _hip.ptr(self.flat_grad), _hip.ptr(self.exp_avg),
                  _hip.ptr(self.exp_avg_sq), self.numel, self.step_count, self.lr, self.betas[0], self.betas[1],
                  self.eps, self.weight_decay, float(grad_scale), _hip.stream())

    def step_from_rows(self, part: torch.Tensor, grad_scale: float = 1.0) -> None:
        """``flat_grad = part.sum(0)`` (one gradient row per clip, the order of ``mx_reduce_rows``) and the AdamW step in ONE
        launch -- the TBPTT loop of the effect model takes 83 optimizer steps per batch on 17 473 parameters.  Bit-identical
        to ``mx_reduce_rows`` followed by ``step()``; with a clip set it IS those launches (the norm needs the whole summed
        gradient before the first element can be updated)."""
        assert part.dim() == 2 and part.size(1) == self.numel and part.is_contiguous() and part.dtype == torch.float32
        self.step_count += 1
        if self.clip_val is not None:
            _hip.call("mx_reduce_rows", _hip.ptr(part), part.size(0), self.numel, 0, _hip.ptr(self.flat_grad), _hip.stream())
            return self._step_clip(grad_scale)
        _hip.call("mx_reduce_rows_adamw_step", _hip.ptr(part), part.size(0), _hip.ptr(self.flat_param), _hip.ptr(self.flat_grad),
                  _hip.ptr(self.exp_avg), _hip.ptr(self.exp_avg_sq), self.numel, self.step_count, self.lr, self.betas[0],
                  self.betas[1], self.eps, self.weight_decay, float(grad_scale), _hip.stream())

    def state_dict(self) -> Dict[str, object]:
        return {"step": self.step_count, "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(),
                "lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay,
                "clip_val": self.clip_val, "clip_algorithm": self.clip_algorithm}

    def load_state_dict(self, sd: Dict[str, object]) -> None:
        self.step_count = int(sd["step"])
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        if "clip_val" in sd:                    # absent in state dicts written before the clip existed
            self.set_gradient_clip(sd["clip_val"], sd.get("clip_algorithm", "norm"))

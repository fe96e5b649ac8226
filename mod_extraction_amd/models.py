"""Host mirror of mod_extraction/models.py: same classes, constructor arguments, forward signatures
and state-dict keys; every forward/backward runs hand-written HIP kernels through the C ABI.

* ``Spectral2DCNN`` (models.py:128-215): log-mel front end (``mx_logmel_fwd``) and six fused
  LayerNorm -> Conv2d(5x13) -> MaxPool(2,1) -> PReLU blocks on the fp32 matrix cores
  (``mx_conv_block_{fwd,dgrad,wgrad}``, ``mx_plane_stats``, ``mx_ln_prelu_bwd``), head
  (``mx_head_{fwd,bwd}``), wired into autograd by one ``torch.autograd.Function``.
  The ``torch.nn`` layer objects inside ``self.cnn`` / ``self.output`` are parameter holders only
  (they give the reference's state-dict keys and default initialisation); they are never called.
* ``LSTMEffectModel`` / ``HiddenStateModel`` (models.py:292-339) and ``RandomLFO`` (models.py:19-69).
"""
import logging
import math
import os
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor as T, nn

from . import _hip

log = logging.getLogger(__name__)

# Arithmetic of the 64->64 channel convolutions (forward + data gradient):
#   "f16x3"  fp16 matrix cores on split operands (hi + lo pairs, 3 MFMAs per product group) -- fp32-equivalent
#            accuracy (csrc/conv_f16.hip), 5.3x the fp32 MFMA rate;   "f32"  exact fp32 MFMA (csrc/conv2d.hip).
CONV_PRECISION = os.environ.get("MODEX_CONV_PRECISION", "f16x3")
# set to a dict to capture the backward's intermediates: G{l} (fp32 dL/dp of block l, where it exists), amax{l}, p{l}, dxhat{l}
# (oracle.models.forward_routed replays the recorded decisions; tests/test_gpu_cnn.py, __graft_entry__.smoke)
DEBUG_TAP = None
PITCH = 352            # activation row pitch (floats); 345 frames + pad (csrc/conv_common.h)
LN_EPS = 1e-5          # torch.nn.LayerNorm default


# ---------------------------------------------------------------------------------------------
# mel front-end constants (torchaudio 0.13.1 MelSpectrogram defaults as used at models.py:170-175)
# ---------------------------------------------------------------------------------------------
def htk_mel_filterbank(n_freqs: int, f_min: float, f_max: float, n_mels: int, sample_rate: int) -> T:
    """torchaudio.functional.melscale_fbanks(norm=None, mel_scale='htk'): triangular filters."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    m_min = 2595.0 * math.log10(1.0 + (f_min / 700.0))
    m_max = 2595.0 * math.log10(1.0 + (f_max / 700.0))
    m_pts = torch.linspace(m_min, m_max, n_mels + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down_slopes = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up_slopes = slopes[:, 2:] / f_diff[1:]
    return torch.max(torch.zeros(1), torch.min(down_slopes, up_slopes))


def _band_limits(fb: T) -> Tuple[T, T]:
    nz = fb != 0
    any_nz = nz.any(dim=0)
    idx = torch.arange(fb.size(0)).unsqueeze(1).expand_as(fb)
    lo = torch.where(nz, idx, torch.full_like(idx, fb.size(0))).min(dim=0).values
    hi = torch.where(nz, idx + 1, torch.zeros_like(idx)).max(dim=0).values
    lo = torch.where(any_nz, lo, torch.zeros_like(lo))
    return lo.to(torch.int32), hi.to(torch.int32)


class _Buffers(nn.Module):
    """Plain namespace module (gives buffers their torchaudio state-dict key prefixes)."""


class MelSpectrogramHIP(nn.Module):
    """State-dict compatible stand-in for torchaudio's MelSpectrogram (keys
    ``spectrogram.window`` and ``mel_scale.fb``); the transform itself is the HIP kernel."""

    def __init__(self, sample_rate: int, n_fft: int, hop_length: int, n_mels: int) -> None:
        super().__init__()
        if n_fft not in (512, 1024, 2048):
            raise NotImplementedError("mx_logmel_fwd is built for n_fft in {512, 1024, 2048}")
        self.sample_rate, self.n_fft, self.hop_length, self.n_mels = sample_rate, n_fft, hop_length, n_mels
        self.spectrogram = _Buffers()
        self.spectrogram.register_buffer("window", torch.hann_window(n_fft))
        self.mel_scale = _Buffers()
        self.mel_scale.register_buffer("fb", htk_mel_filterbank(n_fft // 2 + 1, 0.0, float(sample_rate // 2),
                                                                n_mels, sample_rate))
        k = torch.arange(n_fft, dtype=torch.float64) * (-2.0 * math.pi / n_fft)
        self.register_buffer("twiddle", torch.stack([torch.cos(k), torch.sin(k)], dim=1).float(), persistent=False)
        self._bands: Optional[Tuple[T, T, int]] = None

    def bands(self) -> Tuple[T, T]:
        fb = self.mel_scale.fb
        if self._bands is None or self._bands[2] != fb._version or self._bands[0].device != fb.device:
            lo, hi = _band_limits(fb.detach().cpu())
            self._bands = (lo.to(fb.device), hi.to(fb.device), fb._version)
        return self._bands[0], self._bands[1]

    def log_mel(self, x: T, n_frames: int, eps: float, masks: Sequence[int] = (0, 0, 0, 0), pitch: int = PITCH) -> T:
        """x (B, C, N) -> (B, C, n_mels, pitch) = log(clip(mel, eps)) with SpecAugment ranges."""
        B, C, N = x.shape
        xc = x.contiguous().float()
        out = torch.empty((B, C, self.n_mels, pitch), device=x.device, dtype=torch.float32)
        lo, hi = self.bands()
        f0, f1, t0, t1 = (int(v) for v in masks)
        _hip.call("mx_logmel_fwd", _hip.ptr(xc), B * C, N, _hip.ptr(self.spectrogram.window), _hip.ptr(self.twiddle),
                  _hip.ptr(self.mel_scale.fb), _hip.ptr(lo), _hip.ptr(hi), self.n_fft, self.hop_length, self.n_mels,
                  n_frames, pitch, float(eps), f0, f1, t0, t1, _hip.ptr(out), _hip.stream())
        return out


def specaugment_bounds(size: int, mask_param: int) -> Tuple[int, int]:
    """torchaudio.functional.mask_along_axis: one mask per batch; two host ``torch.rand(1)`` draws
    (value, then min_value); masked range [int(min_value), int(min_value) + int(value))."""
    value = torch.rand(1) * mask_param
    min_value = torch.rand(1) * (size - value)
    start = int(min_value.long())
    return start, start + int(value.long())


# ---------------------------------------------------------------------------------------------
# the CNN stack as one autograd node
# ---------------------------------------------------------------------------------------------
# first block on the fp16 pipes too (MODEX_BLOCK1=f32 keeps it on the exact-fp32 MFMA kernel; A/B knob)
BLOCK1_F16 = os.environ.get("MODEX_BLOCK1", "f16x3") != "f32"
# weight gradient of the 64-channel blocks: sparse (2:4 along the pooling pair) or dense matrix instruction
WGRAD_SPARSE = os.environ.get("MODEX_WGRAD", "sparse") != "dense"
WGRAD_SPARSE_MAX_T = int(os.environ.get("MODEX_WGRAD_SP_MAXT", "4"))     # dilations above it: dense kernel (no shared fragment blocks)
DGRAD_SPARSE = os.environ.get("MODEX_DGRAD", "sparse") != "dense"
DIRECT_GRADS = os.environ.get("MODEX_DIRECT_GRADS", "1") != "0"   # parameter gradients written straight into FlatAdamW's flat buffer
STATS_FUSED = os.environ.get("MODEX_STATS", "fused") != "sweep"   # next block's LayerNorm statistics from the forward epilogue
# LayerNorm / PReLU backward written straight into the pooled operand of the block below (blocks whose two gradients both run
# on the sparse instruction): dL/dp never exists in fp32.  "split" keeps the two passes (A/B knob).
GPOOL_FUSED = os.environ.get("MODEX_GPOOL", "fused") != "split"
LN_FUSED = os.environ.get("MODEX_LN", "fused") != "sweep"      # LayerNorm-backward statistics from the data-gradient epilogue
# the gradient of the first block handed to its weight gradient as f16x3 pairs (written in place by the LayerNorm backward, scale
# from the bound on max|G|) instead of fp32 values that the weight gradient scales / splits while staging ("0": round-4 route)
BLOCK1_PAIR = os.environ.get("MODEX_BLOCK1_PAIR", "1") != "0"

# workspace sizes in elements; KH / KW / TAPS / CO are CV_KH / CV_KW / CV_TAPS / CV_CO of csrc/conv_common.h
KH, KW, TAPS, CO = 5, 13, 65, 64
W_F16_ELEMS = 4 * KH * KW * CO * 16              # [ci / 16][kh][kw][khalf][co][8]: pack_weights_f16_kernel (csrc/conv_f16.hip)
W_KVEC_ELEMS = KW * 2 * CO * 8                   # [kw][khalf][co][8], k = 2 kh + ci: pack_weights_kvec_f16_kernel (csrc/conv_f16.hip)
W_SP_ELEMS = 4 * 3 * 2 * KW * 2 * 64 * 16        # [cb][m][r][kwf][ci tile][lane][16]: pack_weights_sp_f16_kernel (csrc/dgrad_sp_f16.hip)
KVEC_PART_ELEMS = KW * CO * 16                   # per slab, (tap column, co, k): wgrad_kvec_f16_kernel (csrc/wgrad_kvec_f16.hip)
WS_ROW_KS = 22                                   # WS_ROW_KS of csrc/wgrad_sp_f16.hip: index words per pooled row of 352 positions


def _wgrad_part(n_slabs: int, cin: int, dev) -> T:
    """Per-slab partial sums (TAPS, CO, cin) of the 5 x 13 weight-gradient kernels (csrc/wgrad*.hip), reduced in fp64 by them."""
    return torch.empty(n_slabs * TAPS * CO * cin, device=dev, dtype=torch.float32)


def _slabs(rows: int, n_target: int) -> Tuple[int, int]:
    """(rows per slab, slabs) when a weight gradient deals `rows` rows to about n_target workgroups per kernel row."""
    rps = max(1, -(-rows // n_target))
    return rps, -(-rows // rps)


def _f16_pair(dev, *shape: int) -> Tuple[T, T]:
    """The (hi, lo) halves of an f16x3 operand."""
    return (torch.empty(shape, device=dev, dtype=torch.float16), torch.empty(shape, device=dev, dtype=torch.float16))


def _f32(dev, *shape: int) -> T:
    return torch.empty(shape, device=dev, dtype=torch.float32)


def _pack(w: T, flip: int) -> T:
    out = _f32(w.device, w.numel())
    _hip.call("mx_conv_pack_weights", _hip.ptr(w.contiguous()), w.size(0), w.size(1), flip, _hip.ptr(out),
              _hip.stream())
    return out


def _pack_f16(w: T, flip: int) -> Tuple[T, T]:
    hi, lo = _f16_pair(w.device, W_F16_ELEMS)
    _hip.call("mx_conv_pack_weights_f16", _hip.ptr(w.contiguous()), flip, _hip.ptr(hi), _hip.ptr(lo), _hip.stream())
    return hi, lo


def _reduce_rows(part: T, rows: int, cols: int, out: Optional[T] = None) -> T:
    if out is None:
        out = _f32(part.device, cols)
    _hip.call("mx_reduce_rows", _hip.ptr(part), rows, cols, 0, _hip.ptr(out), _hip.stream())
    return out


def _direct_grad_views(params) -> Optional[List[T]]:
    """The parameters' ``.grad`` tensors when the backward pass may write its results straight into them: all of them are
    contiguous views of ONE flat gradient buffer (optim.FlatAdamW) and the caller has armed the in-place path for THIS
    backward (``with optimizer.direct_backward(): loss.backward()`` -- ``_modex_fresh`` on the buffer, set on entry, consumed
    here, cleared on exit; ``Trainer.train_step`` does it for the first backward after ``zero_grad()``).  autograd then gets
    ``None`` for those inputs and skips its 20 ``grad += g`` launches per step.  Any other situation -- no flat buffer, a
    backward outside such a scope (weight penalties, a second sub-batch, ``torch.autograd.grad``), plain ``torch.optim`` --
    keeps the ordinary accumulate path, so nothing already in ``.grad`` is ever overwritten silently."""
    views = []
    base = None
    for p in params:
        if not (p.is_leaf and p.requires_grad):          # (.grad of a non-leaf tensor warns)
            return None
        g = p.grad
        if g is None or not g.is_contiguous() or g._base is None or g.dtype != torch.float32:
            return None
        if base is None:
            base = g._base
        elif g._base is not base:
            return None
        views.append(g)
    if base is None or not getattr(base, "_modex_fresh", False):
        return None
    base._modex_fresh = False
    return views


# ---------------------------------------------------------------------------------------------
# the route table: which kernels each block runs and what it receives from the block above
# ---------------------------------------------------------------------------------------------
class BlockRoute(NamedTuple):
    """Everything the forward and the backward of one block branch on.  plan_stack() is the only place that reads the knobs."""
    fwd: str                 # "f16x3": mx_conv_block_fwd_f16 | "kvec": mx_conv_block1_fwd_f16 (first block) | "f32": mx_conv_block_fwd
    stats: str               # LayerNorm statistics: "sweep" (mx_plane_stats) | "epilogue" (mx_plane_stats_finish of the block above's sums)
    leaves_stats: bool       # this block's forward epilogue leaves the sums for the next block's statistics
    g_in: str                # gradient arriving from above: "f32" | "f32+gmax" (max|G| cell ready) | "pooled" (channels-last pair,
    #                          dL/dp never in fp32) | "pair" (f16x3 pairs in place of the fp32 values, first block only)
    operand: Optional[str]   # the forward's f16 operand pair in the backward: "kept" by the forward | "rederived" | None (not used)
    wgrad: str               # "sparse" | "dense" (64-channel f16x3) | "kvec_pair" | "kvec_scaled" (first block) | "f32"
    routed_pair: bool        # the full-resolution routed gradient pair is built (a dense f16x3 kernel consumes it)
    dgrad: Optional[str]     # "sparse+ln" (epilogue leaves the LayerNorm-backward statistics) | "sparse" | "dense" | "f32" | None (block 0)
    ln_bwd: Optional[str]    # gradient for the block below: "gpool" (mx_ln_prelu_bwd_gpool_f16) | "pair" (mx_ln_prelu_bwd_pair) |
    #                          "plain+gmax" | "plain" (mx_ln_prelu_bwd with / without the max|G| cell; it takes ln_part iff
    #                          dgrad == "sparse+ln") | None (block 0)

    @property
    def dgrad_sparse(self) -> bool:
        return self.dgrad in ("sparse", "sparse+ln")


def plan_stack(cin0: int, dilations: Sequence[int], precision: str, n_frames: int,
               operands_kept: bool = True) -> Tuple[BlockRoute, ...]:
    """The route of every block, from the configuration and the module knobs as they are NOW; touches no tensor.
    operands_kept=False plans a backward that finds the forward's operand pairs gone (_CNNStack.backward)."""
    n = len(dilations)
    fits = n_frames <= PITCH - 1                # the sparse kernels take at most PITCH - 1 frames; the full pitch goes dense
    blocks = []                                 # per block, without what depends on its neighbours
    for l, t in enumerate(int(t) for t in dilations):
        if precision == "f16x3" and (cin0 if l == 0 else CO) == 64:
            # sparse matrix instruction: the pooled gradient is the compressed operand, the argmax its index bits.  Weight
            # gradient: dilations <= 4 (for >= 8 the taps share no fragment blocks: dense kernel on the routed full-resolution
            # pair); data gradient: every dilation
            sp_w = WGRAD_SPARSE and t <= WGRAD_SPARSE_MAX_T and fits
            sp_d = DGRAD_SPARSE and fits
            dgrad = ("sparse+ln" if LN_FUSED else "sparse") if sp_d else "dense"
            blocks.append(dict(fwd="f16x3", operand="kept" if operands_kept else "rederived", wgrad="sparse" if sp_w else "dense",
                               routed_pair=not sp_w or (l > 0 and not sp_d), dgrad=dgrad if l > 0 else None))
        elif precision == "f16x3" and l == 0 and cin0 == 2 and BLOCK1_F16 and t == 1:
            # (the k-vector kernel is built for the undilated first block of every shipped config; a dilated one is "f32")
            blocks.append(dict(fwd="kvec", operand=None, wgrad="f32", routed_pair=False, dgrad=None))
        else:
            blocks.append(dict(fwd="f32", operand=None, wgrad="f32", routed_pair=False, dgrad="f32" if l > 0 else None))
    for l, b in enumerate(blocks):
        b["stats"] = "epilogue" if l > 0 and blocks[l - 1]["leaves_stats"] else "sweep"
        b["leaves_stats"] = STATS_FUSED and l + 1 < n and b["fwd"] != "f32"     # (the head takes the last block's output as it is)
    # the gradient chain, from the head down: how block l's LayerNorm / PReLU backward hands dL/dp to block l - 1
    blocks[-1]["g_in"] = "f32+gmax" if blocks[-1]["fwd"] == "f16x3" else "f32"     # mx_head_bwd takes max|G| while it writes G
    kvec_kept = blocks[0]["fwd"] == "kvec" and operands_kept
    for l in range(n - 1, 0, -1):
        b, below = blocks[l], blocks[l - 1]
        pooled_only = l > 1 and below["wgrad"] == "sparse" and below["dgrad"] in ("sparse", "sparse+ln")
        if b["dgrad"] == "sparse+ln" and GPOOL_FUSED and pooled_only:
            b["ln_bwd"], below["g_in"] = "gpool", "pooled"
        elif b["dgrad"] == "sparse+ln" and BLOCK1_PAIR and l == 1 and kvec_kept:
            b["ln_bwd"], below["g_in"] = "pair", "pair"
        elif below["fwd"] == "f16x3" or (l == 1 and kvec_kept):
            b["ln_bwd"], below["g_in"] = "plain+gmax", "f32+gmax"
        else:
            b["ln_bwd"], below["g_in"] = "plain", "f32"
    blocks[0]["ln_bwd"] = None
    if kvec_kept and blocks[0]["g_in"] != "f32":          # the k-vector weight gradient consumes the forward's own operand
        blocks[0].update(operand="kept", wgrad="kvec_pair" if blocks[0]["g_in"] == "pair" else "kvec_scaled")
    return tuple(BlockRoute(**b) for b in blocks)


# ---------------------------------------------------------------------------------------------
# the CNN stack as one autograd node: step functions, one per launch group, then the node
# ---------------------------------------------------------------------------------------------
class _Act(NamedTuple):
    """What a block's forward hands to the next one."""
    p: T                                  # (B, C, H, PITCH) pooled pre-activation (the log-mel planes for the first block)
    slope: Optional[T] = None             # PReLU slope applied to p by its consumer
    bias: Optional[T] = None              # the statistics sums below are taken of PReLU(out) - PReLU(bias)
    stats_part: Optional[T] = None        # {sum, sum of squares} per pooled row from the forward epilogue (leaves_stats)


class _Grad(NamedTuple):
    """What the head / a block's LayerNorm backward hands to the block below, in the form that block's route.g_in names."""
    G: Optional[T] = None                 # fp32 dL/dp ("f32", "f32+gmax"), or the f16x3 pairs written in its place ("pair")
    gmax: Optional[T] = None              # the atomic-max cell holding max|G| bits ("f32+gmax")
    pooled: Optional[tuple] = None        # (gc_hi, gc_lo, gc_idx, gidx, scale) ("pooled")
    pair_scale: Optional[T] = None        # ("pair")
    bsum: Optional[T] = None              # bias-gradient partials (B, 64); the head leaves none


class _Split(NamedTuple):
    """What a block's weight-gradient step leaves for its data gradient."""
    G: Optional[T] = None                 # fp32 gradient (dgrad "f32")
    dz: Tuple[Optional[T], Optional[T]] = (None, None)      # routed full-resolution pair (dgrad "dense")
    gc: Tuple[Optional[T], ...] = (None, None, None)        # pooled channels-last pair + index words (dgrad "sparse*")
    scale: Optional[T] = None
    x16: Tuple[Optional[T], Optional[T]] = (None, None)     # the forward operand, read again by the "sparse+ln" epilogue


class _ParamGrads:
    """Where parameter gradients go: straight into the .grad views (direct) or into fresh tensors handed to autograd."""

    def __init__(self, n: int, direct: Optional[List[T]]) -> None:
        self.direct, self.grads = direct, [None] * n

    def weight(self, i: int, w: T) -> T:
        self.grads[i] = self.direct[i] if self.direct is not None else torch.empty_like(w)
        return self.grads[i]

    def reduce(self, i: int, part: T, rows: int, cols: int) -> None:
        self.grads[i] = _reduce_rows(part, rows, cols, self.direct[i].view(-1) if self.direct is not None else None)

    def for_autograd(self) -> List[Optional[T]]:
        return [None] * len(self.grads) if self.direct is not None else self.grads     # in place: nothing to accumulate


def _block_fwd(r: BlockRoute, x: _Act, w: T, b: T, a: T, n_frames: int, t: int, first: bool):
    """LayerNorm statistics -> (operand prep) -> convolution + max-pool.  Returns (the next block's input, what the backward
    saves, the f16 operand pair or None)."""
    B, cin, H, _ = x.p.shape
    dev, st = x.p.device, _hip.stream()
    stats = _f32(dev, B, cin, 2)
    if r.stats == "epilogue":
        _hip.call("mx_plane_stats_finish", _hip.ptr(x.stats_part), _hip.ptr(x.bias), _hip.ptr(x.slope), B, cin, H,
                  n_frames, LN_EPS, _hip.ptr(stats), st)
    else:
        _hip.call("mx_plane_stats", _hip.ptr(x.p), _hip.ptr(x.slope), B, cin, H, n_frames, LN_EPS, _hip.ptr(stats), st)
    a_out = a.contiguous()
    p = _f32(dev, B, 64, H // 2, PITCH)
    amax = torch.empty((B, 64, H // 2, PITCH), device=dev, dtype=torch.uint8)
    stats_part = _f32(dev, B, H // 2, 64, 2) if r.leaves_stats else None
    operand = None
    if r.fwd == "f16x3":
        operand = _f16_pair(dev, B, H, 4, PITCH, 16)
        _hip.call("mx_conv_prep_fwd_f16", _hip.ptr(x.p), _hip.ptr(stats), _hip.ptr(x.slope), B, H, n_frames,
                  _hip.ptr(operand[0]), _hip.ptr(operand[1]), st)
        w_hi, w_lo = _pack_f16(w, 0)
        _hip.call("mx_conv_block_fwd_f16", _hip.ptr(operand[0]), _hip.ptr(operand[1]), _hip.ptr(w_hi), _hip.ptr(w_lo),
                  _hip.ptr(b.contiguous()), B, H, n_frames, t, _hip.ptr(p), _hip.ptr(amax),
                  _hip.ptr(a_out) if r.leaves_stats else None, _hip.ptr(stats_part), st)
    elif r.fwd == "kvec":
        # first block: (kernel row, channel) pairs are the operand's 16 channels; one K stage
        operand = _f16_pair(dev, B, H, 1, PITCH, 16)
        _hip.call("mx_conv_prep_fwd_kvec_f16", _hip.ptr(x.p), _hip.ptr(stats), B, H, n_frames, _hip.ptr(operand[0]),
                  _hip.ptr(operand[1]), st)
        wk_hi, wk_lo = _f16_pair(dev, W_KVEC_ELEMS)
        _hip.call("mx_conv_pack_weights_kvec_f16", _hip.ptr(w.detach().contiguous()), _hip.ptr(wk_hi), _hip.ptr(wk_lo), st)
        _hip.call("mx_conv_block1_fwd_f16", _hip.ptr(operand[0]), _hip.ptr(operand[1]), _hip.ptr(wk_hi), _hip.ptr(wk_lo),
                  _hip.ptr(b.contiguous()), B, H, n_frames, _hip.ptr(p), _hip.ptr(amax),
                  _hip.ptr(a_out) if r.leaves_stats else None, _hip.ptr(stats_part), st)
    else:
        wt = _pack(w, 0)
        _hip.call("mx_conv_block_fwd", _hip.ptr(x.p), _hip.ptr(stats), _hip.ptr(x.slope), _hip.ptr(wt),
                  _hip.ptr(b.contiguous()), B, cin, H, n_frames, t, 1 if first else 0, _hip.ptr(p), _hip.ptr(amax), st)
    return _Act(p, a_out, b.contiguous(), stats_part), (x.p, stats, amax), operand


def _head_bwd(r_last: BlockRoute, p_last: T, slope_last: T, wout: T, latent: T, out: T, d_out: T, d_latent: Optional[T],
              n_frames: int, gmax_cell: T, pg: _ParamGrads, i_wout: int, i_slope: int) -> _Grad:
    """Head backward: dL/dp of the last block (with max|G| for its f16x3 scale, taken while G is written: no sweep) and the
    gradients of the head's weight and bias and of the last PReLU slope."""
    B, L, Hl, dev = out.size(0), out.size(1), p_last.size(2), out.device
    G = torch.empty_like(p_last)
    dw_part, db_part, ds_part = _f32(dev, B, L * 64), _f32(dev, B, L), _f32(dev, B, 64)
    gmax = gmax_cell if r_last.g_in == "f32+gmax" else None
    _hip.call("mx_head_bwd", _hip.ptr(p_last), _hip.ptr(slope_last), _hip.ptr(wout.contiguous()),
              _hip.ptr(latent), _hip.ptr(out), _hip.ptr(d_out), _hip.ptr(d_latent), B, 64, Hl, n_frames, L,
              _hip.ptr(G), _hip.ptr(dw_part), _hip.ptr(db_part), _hip.ptr(ds_part), _hip.ptr(gmax), _hip.stream())
    pg.reduce(i_wout, dw_part, B, L * 64)
    pg.grads[i_wout] = pg.grads[i_wout].view_as(wout)
    pg.reduce(i_wout + 1, db_part, B, L)
    pg.reduce(i_slope, ds_part, B, 64)
    return _Grad(G=G, gmax=gmax)


def _wgrad_f16x3(r: BlockRoute, l: int, g: _Grad, kept: dict, x_in: T, stats: T, amax: T, slope_prev: Optional[T],
                 n_frames: int, t: int, dW: T) -> _Split:
    """Weight gradient of a 64-channel f16x3 block: gradient operands (unless they arrive pooled), the forward's operand pair
    (kept, or derived again), then the sparse kernel on the pooled pair or the dense one on the routed pair."""
    B, _, H, _ = x_in.shape
    Hp, dev, st = H // 2, x_in.device, _hip.stream()
    dz = _f16_pair(dev, B, H, 4, PITCH, 16) if r.routed_pair else (None, None)
    if r.g_in == "pooled":
        gc_hi, gc_lo, gc_idx, gidx, scale = g.pooled         # made by the LayerNorm backward of the block above
    else:
        ready = r.g_in == "f32+gmax"
        ws = g.gmax if ready else torch.empty(1, device=dev, dtype=torch.int32)
        scale = _f32(dev, 2)
        _hip.call("mx_conv_prep_dgrad_f16", _hip.ptr(g.G), _hip.ptr(amax), B, H, n_frames, _hip.ptr(ws),
                  1 if ready else 0, _hip.ptr(scale), _hip.ptr(dz[0]), _hip.ptr(dz[1]), st)
        gc_hi = gc_lo = gc_idx = gidx = None
        if r.wgrad == "sparse" or r.dgrad_sparse:
            # one pass over G: the channels-last pooled pair both sparse kernels read, the data gradient's index
            # words and (for the weight gradient) the planar ones
            gc_hi, gc_lo = _f16_pair(dev, B, Hp, 4, PITCH, 16)
            gc_idx = torch.empty((B, Hp, 4, PITCH), device=dev, dtype=torch.int32)
            if r.wgrad == "sparse":
                gidx = torch.empty((B, 64, Hp, WS_ROW_KS, 2), device=dev, dtype=torch.int16)
            _hip.call("mx_conv_prep_gpool_cl_f16", _hip.ptr(g.G), _hip.ptr(amax), _hip.ptr(scale), B, H, n_frames,
                      _hip.ptr(gc_hi), _hip.ptr(gc_lo), _hip.ptr(gc_idx), _hip.ptr(gidx), st)
    if r.operand == "kept":
        x_hi, x_lo = kept.pop(l)              # released when its last consumer (this step, or the data gradient) has been launched
    else:
        x_hi, x_lo = _f16_pair(dev, B, H, 4, PITCH, 16)
        _hip.call("mx_conv_prep_fwd_f16", _hip.ptr(x_in), _hip.ptr(stats), _hip.ptr(slope_prev), B, H, n_frames,
                  _hip.ptr(x_hi), _hip.ptr(x_lo), st)
    # 256 slabs x 5 kernel rows = 5 full rounds of 256 workgroups
    rps, n_slabs = _slabs(B * Hp if r.wgrad == "sparse" else B * H, 256)
    part = _wgrad_part(n_slabs, 64, dev)
    if r.wgrad == "sparse":
        _hip.call("mx_conv_block_wgrad_sp_f16", _hip.ptr(gc_hi), _hip.ptr(gc_lo), _hip.ptr(gidx), _hip.ptr(x_hi),
                  _hip.ptr(x_lo), _hip.ptr(scale), B, H, n_frames, t, rps, _hip.ptr(part), _hip.ptr(dW), st)
    else:
        _hip.call("mx_conv_block_wgrad_f16", _hip.ptr(dz[0]), _hip.ptr(dz[1]), _hip.ptr(x_hi), _hip.ptr(x_lo),
                  _hip.ptr(scale), B, H, t, rps, _hip.ptr(part), _hip.ptr(dW), st)
    return _Split(dz=dz if r.dgrad == "dense" else (None, None), gc=(gc_hi, gc_lo, gc_idx), scale=scale,
                  x16=(x_hi, x_lo) if r.dgrad == "sparse+ln" else (None, None))


def _weight_grad(r: BlockRoute, l: int, g: _Grad, kept: dict, x_in: T, stats: T, amax: T, slope_prev: Optional[T],
                 n_frames: int, t: int, dW: T) -> _Split:
    if r.fwd == "f16x3":
        return _wgrad_f16x3(r, l, g, kept, x_in, stats, amax, slope_prev, n_frames, t, dW)
    B, cin, H, _ = x_in.shape
    dev, st = x_in.device, _hip.stream()
    if r.wgrad in ("kvec_pair", "kvec_scaled"):
        # first block on the fp16 pipes: the kept k-vector operand; the gradient is routed while staging and arrives either as
        # f16x3 pairs (mx_ln_prelu_bwd_pair) or in fp32 with its max|G| cell (then scaled / split on the fly too)
        xk_hi, xk_lo = kept.pop(l)
        rps, n_slabs = _slabs(B * H, 2048)
        part = _f32(dev, n_slabs * KVEC_PART_ELEMS)
        if r.wgrad == "kvec_pair":
            _hip.call("mx_conv_block1_wgrad_pair_f16", _hip.ptr(g.G), _hip.ptr(amax), _hip.ptr(g.pair_scale), _hip.ptr(xk_hi),
                      _hip.ptr(xk_lo), B, H, n_frames, rps, _hip.ptr(part), _hip.ptr(dW), st)
        else:
            scale1 = _f32(dev, 2)
            _hip.call("mx_conv_block1_wgrad_f16", _hip.ptr(g.G), _hip.ptr(amax), _hip.ptr(g.gmax), _hip.ptr(xk_hi),
                      _hip.ptr(xk_lo), B, H, n_frames, rps, _hip.ptr(scale1), _hip.ptr(part), _hip.ptr(dW), st)
    else:
        rps, n_slabs = _slabs(B * H, 256 if cin == 64 else 1024)
        part = _wgrad_part(n_slabs, cin, dev)
        _hip.call("mx_conv_block_wgrad", _hip.ptr(g.G), _hip.ptr(amax), _hip.ptr(x_in), _hip.ptr(stats),
                  _hip.ptr(slope_prev), B, cin, H, n_frames, t, rps, _hip.ptr(part), _hip.ptr(dW), st)
    return _Split(G=g.G)


def _data_grad(r: BlockRoute, l: int, d: _Split, w: T, amax: T, B: int, H: int, n_frames: int, t: int, zws: T):
    """dL/dxhat of block l > 0.  Returns (dxhat, ln_part, gx_bits): with dgrad "sparse+ln" the epilogue also leaves the plane
    statistics of the LayerNorm backward below (x = xhat) and, when that pass needs its scale before it runs ("gpool",
    "pair"), max|dxhat| / max|xhat| in the block's first two atomic-max cells."""
    dev, st = w.device, _hip.stream()
    dxhat = _f32(dev, B, 64, H, PITCH)
    ln_part = gx_bits = None
    if r.dgrad_sparse:
        # sparse matrix instruction, transposed tiles: pooled channels-last gradient x fragment-packed weights
        ws_hi, ws_lo = _f16_pair(dev, W_SP_ELEMS)
        _hip.call("mx_conv_pack_weights_sp_f16", _hip.ptr(w.detach().contiguous()), _hip.ptr(ws_hi), _hip.ptr(ws_lo), st)
        if r.dgrad == "sparse+ln":
            ln_part = _f32(dev, B, 64, H, 2, 2)
            gx_bits = zws[4 * l:4 * l + 2] if r.ln_bwd in ("gpool", "pair") else None
        _hip.call("mx_conv_block_dgrad_sp_f16", _hip.ptr(d.gc[0]), _hip.ptr(d.gc[1]), _hip.ptr(d.gc[2]),
                  _hip.ptr(ws_hi), _hip.ptr(ws_lo), _hip.ptr(d.scale), B, H, n_frames, t,
                  _hip.ptr(dxhat), _hip.ptr(d.x16[0]), _hip.ptr(d.x16[1]), _hip.ptr(ln_part), _hip.ptr(gx_bits), st)
    elif r.dgrad == "dense":
        w_hi, w_lo = _pack_f16(w, 1)
        _hip.call("mx_conv_block_dgrad_f16", _hip.ptr(d.dz[0]), _hip.ptr(d.dz[1]), _hip.ptr(w_hi), _hip.ptr(w_lo),
                  _hip.ptr(d.scale), B, H, n_frames, t, _hip.ptr(dxhat), st)
    else:
        wt_f = _pack(w, 1)
        _hip.call("mx_conv_block_dgrad", _hip.ptr(d.G), _hip.ptr(amax), _hip.ptr(wt_f), B, H, n_frames, t, _hip.ptr(dxhat), st)
    if DEBUG_TAP is not None:
        DEBUG_TAP[f"dxhat{l}"] = dxhat.clone()
    return dxhat, ln_part, gx_bits


def _ln_prelu_bwd(r: BlockRoute, l: int, x_in: T, dxhat: T, ln_part: Optional[T], gx_bits: Optional[T], stats: T,
                  slope_prev: T, amax_below: T, n_frames: int, zws: T) -> Tuple[_Grad, T]:
    """LayerNorm / PReLU backward of block l > 0: dL/dp of block l - 1 in the form r.ln_bwd names, with that block's bias-gradient
    partials, and the partials of d loss / d slope (returned beside it)."""
    B, _, H, _ = x_in.shape
    dev, st = x_in.device, _hip.stream()
    ds_part, bsum = _f32(dev, B, 64), _f32(dev, B, 64)
    if r.ln_bwd in ("gpool", "pair"):
        # the f16x3 scale must be known before the pass: from a bound on max|G| (csrc/dgrad_sp_f16.hip)
        m12, scale_n = _f32(dev, B, 64, 2), _f32(dev, 2)
        bound_ws = torch.empty(1, device=dev, dtype=torch.int32)
        _hip.call("mx_ln_bwd_finish", _hip.ptr(ln_part), _hip.ptr(stats), _hip.ptr(slope_prev), _hip.ptr(gx_bits),
                  B, 64, H, n_frames, _hip.ptr(m12), _hip.ptr(bound_ws), _hip.ptr(scale_n), st)
    if r.ln_bwd == "gpool":
        # dL/dp of the block below never exists in fp32: LayerNorm / PReLU backward -> scale -> split -> channels-last
        # pooled pair + index words, one pass
        gn_hi, gn_lo = _f16_pair(dev, B, H, 4, PITCH, 16)
        gn_idx = torch.empty((B, H, 4, PITCH), device=dev, dtype=torch.int32)
        gn_pidx = torch.empty((B, 64, H, WS_ROW_KS, 2), device=dev, dtype=torch.int16)
        part2 = _f32(dev, B, 64, H, 6, 2)
        _hip.call("mx_ln_prelu_bwd_gpool_f16", _hip.ptr(x_in), _hip.ptr(dxhat), _hip.ptr(amax_below),
                  _hip.ptr(stats), _hip.ptr(slope_prev), _hip.ptr(m12), _hip.ptr(scale_n), B, H, n_frames,
                  _hip.ptr(gn_hi), _hip.ptr(gn_lo), _hip.ptr(gn_idx), _hip.ptr(gn_pidx), _hip.ptr(part2),
                  _hip.ptr(ds_part), _hip.ptr(bsum), st)
        return _Grad(pooled=(gn_hi, gn_lo, gn_idx, gn_pidx, scale_n), bsum=bsum), ds_part
    if r.ln_bwd == "pair":
        # the first block's gradient as f16x3 pairs, written in place of dxhat
        _hip.call("mx_ln_prelu_bwd_pair", _hip.ptr(x_in), _hip.ptr(dxhat), _hip.ptr(stats), _hip.ptr(slope_prev),
                  B, 64, H, n_frames, _hip.ptr(ds_part), _hip.ptr(bsum), _hip.ptr(ln_part), _hip.ptr(scale_n), st)
        return _Grad(G=dxhat, pair_scale=scale_n, bsum=bsum), ds_part
    gmax = zws[4 * l + 2:4 * l + 3] if r.ln_bwd == "plain+gmax" else None
    _hip.call("mx_ln_prelu_bwd", _hip.ptr(x_in), _hip.ptr(dxhat), _hip.ptr(stats), _hip.ptr(slope_prev),
              B, 64, H, n_frames, _hip.ptr(ds_part), _hip.ptr(bsum), _hip.ptr(gmax), _hip.ptr(ln_part), st)
    return _Grad(G=dxhat, gmax=gmax, bsum=bsum), ds_part


class _CNNStack(torch.autograd.Function):
    """logmel (B,Cin,H,PITCH) -> (sigmoid output (B,L,W), latent (B,64,W)).
    params: [w1,b1,a1, ..., w6,b6,a6, wout, bout].  Which kernels run is read off plan_stack()'s table, nowhere else."""

    @staticmethod
    def forward(ctx, logmel: T, n_frames: int, dilations: Tuple[int, ...], precision: str, *params: T):
        n_blocks = len(dilations)
        routes = plan_stack(logmel.size(1), dilations, precision, n_frames)
        # the fp16 operand pairs the weight gradients consume are kept when a backward pass will follow (5.9 GB at
        # 256 clips x 2 s: cheaper than re-deriving them from the saved activations)
        keep = any(ctx.needs_input_grad)
        ctx.operands = {}
        x, saved = _Act(logmel), []
        for l, r in enumerate(routes):
            x, for_bwd, operand = _block_fwd(r, x, *params[3 * l:3 * l + 3], n_frames, int(dilations[l]), l == 0)
            saved += for_bwd
            if keep and r.operand == "kept":
                ctx.operands[l] = operand
            del operand
        wout, bout = params[3 * n_blocks], params[3 * n_blocks + 1]
        B, H, L, dev = logmel.size(0), x.p.size(2), wout.size(0), logmel.device
        latent, out = _f32(dev, B, 64, n_frames), _f32(dev, B, L, n_frames)
        _hip.call("mx_head_fwd", _hip.ptr(x.p), _hip.ptr(x.slope), _hip.ptr(wout.contiguous()),
                  _hip.ptr(bout.contiguous()), B, 64, H, n_frames, L, _hip.ptr(latent), _hip.ptr(out), _hip.stream())
        ctx.save_for_backward(*saved, x.p, latent, out, *params)
        ctx.param_objs = params               # the Parameter objects themselves: their .grad views are looked up in backward
        ctx.meta = (n_frames, tuple(dilations), n_blocks, precision)
        return out, latent

    @staticmethod
    def backward(ctx, d_out: Optional[T], d_latent: Optional[T]):
        n_frames, dilations, n_blocks, precision = ctx.meta
        tensors = ctx.saved_tensors
        saved, (p_last, latent, out), params = tensors[:3 * n_blocks], tensors[3 * n_blocks:3 * n_blocks + 3], \
            tensors[3 * n_blocks + 3:]
        # Kept-operand rule: the first backward consumes the operand pairs the forward kept and releases each one as soon as its
        # last consumer has been launched.  A second backward through a retained graph finds them gone: it is planned with
        # operands_kept=False, i.e. the 64-channel blocks derive their operands again (mx_conv_prep_fwd_f16) and block 0 takes
        # the exact-fp32 weight gradient (mx_conv_block_wgrad), with the gradient handed to it in plain fp32.
        kept, ctx.operands = ctx.operands, None
        routes = plan_stack(saved[0].size(1), dilations, precision, n_frames, operands_kept=kept is not None)
        B, dev = out.size(0), out.device
        pg = _ParamGrads(len(params), _direct_grad_views(ctx.param_objs) if DIRECT_GRADS else None)
        d_out = (d_out if d_out is not None else torch.zeros_like(out)).contiguous()
        d_latent = d_latent.contiguous() if d_latent is not None else None
        # one zeroed workspace for every atomic-max cell of this backward pass (each used to be its own fill launch): cells
        # 4 l .. 4 l + 3 belong to block l, cell 4 n_blocks to the head
        zws = torch.zeros(4 * (n_blocks + 1), device=dev, dtype=torch.int32)
        g = _head_bwd(routes[-1], p_last, params[3 * (n_blocks - 1) + 2].contiguous(), params[3 * n_blocks], latent, out,
                      d_out, d_latent, n_frames, zws[4 * n_blocks:4 * n_blocks + 1], pg, 3 * n_blocks, 3 * (n_blocks - 1) + 2)
        for l in range(n_blocks - 1, -1, -1):
            r, t = routes[l], int(dilations[l])
            x_in, stats, amax = saved[3 * l:3 * l + 3]
            H = x_in.size(2)
            slope_prev = params[3 * (l - 1) + 2].contiguous() if l > 0 else None
            if DEBUG_TAP is not None:
                if r.g_in in ("f32", "f32+gmax"):      # (G{l} is absent where dL/dp never exists in fp32)
                    DEBUG_TAP[f"G{l}"] = g.G.clone()
                DEBUG_TAP[f"amax{l}"] = amax.clone()
                DEBUG_TAP[f"p{l}"] = (p_last if l == n_blocks - 1 else saved[3 * (l + 1)]).clone()
            # bias gradient: sum of G over (b, h, w), a by-product of the LayerNorm backward above (the head leaves none)
            bsum = g.bsum
            if bsum is None:
                bsum = _f32(dev, B, 64)
                _hip.call("mx_plane_sum", _hip.ptr(g.G), B * 64, H // 2, n_frames, _hip.ptr(bsum), _hip.stream())
            pg.reduce(3 * l + 1, bsum, B, 64)
            d = _weight_grad(r, l, g, kept, x_in, stats, amax, slope_prev, n_frames, t, pg.weight(3 * l, params[3 * l]))
            del g, bsum                          # (these releases decide the peak of a 256-clip step)
            if l == 0:
                break
            dxhat, ln_part, gx_bits = _data_grad(r, l, d, params[3 * l], amax, B, H, n_frames, t, zws)
            del d                                # operand pairs: gone before the LayerNorm backward allocates the next ones
            g, ds_part = _ln_prelu_bwd(r, l, x_in, dxhat, ln_part, gx_bits, stats, slope_prev, saved[3 * (l - 1) + 2],
                                       n_frames, zws)
            del dxhat, ln_part
            pg.reduce(3 * (l - 1) + 2, ds_part, B, 64)
        return (None, None, None, None, *pg.for_autograd())


class Spectral2DCNN(nn.Module):
    def __init__(self,
                 in_ch: int = 1,
                 n_samples: int = 88200,
                 sr: float = 44100,
                 n_fft: int = 1024,
                 hop_len: int = 256,
                 n_mels: int = 256,
                 kernel_size: Tuple[int, int] = (5, 13),
                 out_channels: Optional[List[int]] = None,
                 bin_dilations: Optional[List[int]] = None,
                 temp_dilations: Optional[List[int]] = None,
                 pool_size: Tuple[int, int] = (3, 1),
                 latent_dim: int = 1,
                 freq_mask_amount: float = 0.0,
                 time_mask_amount: float = 0.0,
                 use_ln: bool = True,
                 eps: float = 1e-7) -> None:
        super().__init__()
        if out_channels is None:
            out_channels = [64] * 5
        if bin_dilations is None:
            bin_dilations = [1] * len(out_channels)
        if temp_dilations is None:
            temp_dilations = [2 ** idx for idx in range(len(out_channels))]
        assert len(out_channels) == len(bin_dilations) == len(temp_dilations)
        assert pool_size[1] == 1
        self.sr, self.n_fft, self.hop_len, self.n_mels = sr, n_fft, hop_len, n_mels
        self.kernel_size, self.pool_size, self.latent_dim = tuple(kernel_size), tuple(pool_size), latent_dim
        self.freq_mask_amount, self.time_mask_amount = freq_mask_amount, time_mask_amount
        self.use_ln, self.eps = use_ln, eps
        self.out_channels, self.bin_dilations, self.temp_dilations = list(out_channels), list(bin_dilations), \
            list(temp_dilations)
        self.in_ch = in_ch
        self.n_frames = n_samples // hop_len + 1
        # what the f16x3 / fp32 block kernels are built for (the only configuration the reference ships); everything else -- the
        # class's own defaults included -- runs the general kernels of csrc/cnn_generic.hip (cnn_generic.GenericCNNStack)
        self.generic = (self.kernel_size != (5, 13) or self.pool_size != (2, 1) or not use_ln
                        or any(c != 64 for c in out_channels) or any(d != 1 for d in bin_dilations)
                        or any(d not in (1, 2, 4, 8, 16) for d in temp_dilations) or in_ch not in (1, 2)
                        or self.n_frames > PITCH or n_mels % (2 ** len(out_channels)) != 0 or latent_dim > 4)
        if self.generic:
            n_bins = n_mels
            for _ in out_channels:
                n_bins //= self.pool_size[0]
            if n_bins < 1 or min(self.kernel_size) < 1 or min(self.bin_dilations + self.temp_dilations) < 1 or self.pool_size[0] > 255:
                raise ValueError(f"Spectral2DCNN: {n_mels} mel bins do not survive {len(out_channels)} poolings by "
                                 f"{self.pool_size[0]} (or a kernel size / dilation below 1)")
        self.conv_precision = CONV_PRECISION        # "f16x3" (default) or "f32", see the module header
        self.spectrogram = MelSpectrogramHIP(int(sr), n_fft, hop_len, n_mels)
        self.freq_mask_param = int(freq_mask_amount * n_mels)
        self.time_mask_param = int(time_mask_amount * self.n_frames)
        layers: List[nn.Module] = []
        n_bins, c_in = n_mels, in_ch
        for out_ch, b_dil, t_dil in zip(out_channels, bin_dilations, temp_dilations):
            if use_ln:
                layers.append(nn.LayerNorm([n_bins, self.n_frames], elementwise_affine=False))
            layers.append(nn.Conv2d(c_in, out_ch, self.kernel_size, stride=(1, 1), dilation=(b_dil, t_dil),
                                    padding="same"))
            layers.append(nn.MaxPool2d(kernel_size=self.pool_size))
            layers.append(nn.PReLU(num_parameters=out_ch))
            c_in, n_bins = out_ch, n_bins // self.pool_size[0]
        self.cnn = nn.Sequential(*layers)       # parameter holders; never called
        self.output = nn.Conv1d(out_channels[-1], latent_dim, kernel_size=(1,))

    def _stack_params(self) -> List[T]:
        ps: List[T] = []
        per, first = (4, 1) if self.use_ln else (3, 0)          # module indices as in the reference's nn.Sequential (models.py:184-191)
        for i in range(len(self.out_channels)):
            conv, prelu = self.cnn[per * i + first], self.cnn[per * i + first + 2]
            w = conv.weight
            if i == 0 and self.in_ch == 1 and not self.generic:      # pad the single input channel to the 2-channel kernel
                w = torch.cat([w, torch.zeros_like(w)], dim=1)
            ps += [w, conv.bias, prelu.weight]
        # (the Conv1d's (latent_dim, 64, 1) weight itself, not a 2-D view of it: a view is not a leaf, and its gradient could
        #  not be written in place -- _direct_grad_views; the kernels only need its pointer and first dimension)
        ps += [self.output.weight, self.output.bias]
        return ps

    def draw_masks(self) -> Tuple[int, int, int, int]:
        f0 = f1 = t0 = t1 = 0
        if self.training:
            if self.freq_mask_amount > 0:
                f0, f1 = specaugment_bounds(self.n_mels, self.freq_mask_param)
            if self.time_mask_amount > 0:
                t0, t1 = specaugment_bounds(self.n_frames, self.time_mask_param)
        return f0, f1, t0, t1

    def log_mel(self, x: T, masks: Optional[Sequence[int]] = None) -> T:
        assert x.ndim == 3
        n_frames = x.size(-1) // self.hop_len + 1
        assert n_frames == self.n_frames, "clip length does not match the LayerNorm shape"
        masks = self.draw_masks() if masks is None else masks
        if self.generic:                        # dense (B, in_ch, n_mels, n_frames)
            with torch.no_grad():
                return self.spectrogram.log_mel(x, self.n_frames, self.eps, masks, pitch=self.n_frames)
        if self.in_ch == 1:
            x = torch.cat([x, torch.zeros_like(x)], dim=1)
        with torch.no_grad():
            return self.spectrogram.log_mel(x, self.n_frames, self.eps, masks)

    def forward(self, x: T, masks: Optional[Sequence[int]] = None) -> (T, T):
        logmel = self.log_mel(x, masks)
        if self.generic:
            from .cnn_generic import GenericCNNStack
            cfg = (self.kernel_size, int(self.pool_size[0]), bool(self.use_ln),
                   tuple(zip(self.out_channels, self.bin_dilations, self.temp_dilations)))
            return GenericCNNStack.apply(logmel, cfg, *self._stack_params())
        out, latent = _CNNStack.apply(logmel, self.n_frames, tuple(self.temp_dilations), self.conv_precision,
                                      *self._stack_params())
        return out, latent


class RandomLFO(nn.Module):
    """models.py:19-69: baseline 'extractor' that emits random / perturbed-ground-truth LFOs."""

    def __init__(self,
                 n_samples: int,
                 sr: float,
                 use_shape_gt: bool = False,
                 use_phase_gt: bool = False,
                 use_freq_gt: bool = False,
                 shapes: Optional[List[str]] = None,
                 freq_min: float = 0.5,
                 freq_max: float = 3.0,
                 phase_error: float = 0.0,
                 freq_error: float = 0.0) -> None:
        super().__init__()
        self.n_samples, self.sr = n_samples, sr
        self.use_shape_gt, self.use_phase_gt, self.use_freq_gt = use_shape_gt, use_phase_gt, use_freq_gt
        self.shapes, self.freq_min, self.freq_max = shapes, freq_min, freq_max
        self.phase_error, self.freq_error = phase_error, freq_error

    def forward(self, batch_size: int, fx_params: Optional[Dict[str, T]] = None) -> T:
        from .modulations import make_rand_mod_signal
        shapes_gt = phase_gt = freq_gt = None
        if self.use_shape_gt:
            assert fx_params is not None and "shape" in fx_params
            shapes_gt = fx_params["shape"]
        if self.use_phase_gt:
            assert fx_params is not None and "phase" in fx_params
            phase_gt = fx_params["phase"]
        if self.use_freq_gt:
            assert fx_params is not None and "rate_hz" in fx_params
            freq_gt = fx_params["rate_hz"]
        return make_rand_mod_signal(batch_size, self.n_samples, self.sr, self.freq_min, self.freq_max, shapes_gt,
                                    self.shapes, phase_gt, self.phase_error, freq_gt, self.freq_error).unsqueeze(1)


class SpectrogramHIP(nn.Module):
    """State-dict compatible stand-in for ``torchaudio.transforms.Spectrogram(n_fft, hop_length=hop, normalized=False)``
    (key ``window``; power 2, centre + reflect padding) of SpectralTCN / SpectralDSTCN (models.py:99,252): the log-mel
    kernel with an identity filter bank -- band m = bin m, weight 1.0 -- returns log(clip(|STFT|^2, eps)) exactly."""

    def __init__(self, n_fft: int, hop_length: int) -> None:
        super().__init__()
        if n_fft not in (512, 1024, 2048):
            raise NotImplementedError("mx_logmel_fwd is built for n_fft in {512, 1024, 2048}")
        self.n_fft, self.hop_length, self.n_bins = n_fft, hop_length, n_fft // 2 + 1
        self.register_buffer("window", torch.hann_window(n_fft))
        k = torch.arange(n_fft, dtype=torch.float64) * (-2.0 * math.pi / n_fft)
        self.register_buffer("twiddle", torch.stack([torch.cos(k), torch.sin(k)], dim=1).float(), persistent=False)
        self.register_buffer("eye", torch.eye(self.n_bins), persistent=False)
        self.register_buffer("band_lo", torch.arange(self.n_bins, dtype=torch.int32), persistent=False)
        self.register_buffer("band_hi", torch.arange(1, self.n_bins + 1, dtype=torch.int32), persistent=False)

    def log_power(self, x: T, n_frames: int, eps: float) -> T:
        """x (B, 1, N) -> (B, n_fft/2 + 1, 352) planes = log(clip(power, eps)), columns >= n_frames zero"""
        assert x.ndim == 3 and x.size(1) == 1
        B, _, N = x.shape
        xc = x.contiguous().float()
        out = torch.empty((B, self.n_bins, PITCH), device=x.device, dtype=torch.float32)
        _hip.call("mx_logmel_fwd", _hip.ptr(xc), B, N, _hip.ptr(self.window), _hip.ptr(self.twiddle), _hip.ptr(self.eye),
                  _hip.ptr(self.band_lo), _hip.ptr(self.band_hi), self.n_fft, self.hop_length, self.n_bins, n_frames, PITCH,
                  float(eps), 0, 0, 0, 0, _hip.ptr(out), _hip.stream())
        return out


class SpectralTCN(nn.Module):
    """models.py:72-125: log power spectrogram (513 bins) -> 5-block dilated TCN over time (LayerNorm, 13 taps, PReLU,
    1x1 residual) -> Conv1d(96 -> latent_dim, 1) -> sigmoid; (B, 1, N) -> (B, latent_dim, frames).  The front end and the
    TCN stack run in HIP kernels (``tcn.py``); the 1x1 head + sigmoid is ``mx_binmean_head_*`` at one bin."""

    def __init__(self, n_samples: int = 88200, n_fft: int = 1024, hop_len: int = 256, kernel_size: int = 13,
                 out_channels: Optional[List[int]] = None, dilations: Optional[List[int]] = None, latent_dim: int = 1,
                 use_ln: bool = True, use_res: bool = True, eps: float = 1e-7) -> None:
        super().__init__()
        from .tcn import TCN
        self.n_fft, self.hop_len, self.kernel_size, self.latent_dim = n_fft, hop_len, kernel_size, latent_dim
        self.use_ln, self.use_res, self.eps = use_ln, use_res, eps
        if out_channels is None:
            out_channels = [96] * 5
        self.out_channels = out_channels
        if dilations is None:
            dilations = [2 ** idx for idx in range(len(out_channels))]
        self.dilations = dilations
        self.spectrogram = SpectrogramHIP(n_fft, hop_len)
        self.n_frames = n_samples // hop_len + 1
        self.tcn = TCN(out_channels, dilations, n_fft // 2 + 1, kernel_size, padding=None, use_ln=use_ln,
                       temporal_dims=[self.n_frames] * len(out_channels), use_res=use_res, is_causal=False)
        self.receptive_field = self.tcn.calc_receptive_field()
        log.info(f"Receptive field = {self.receptive_field} samples")
        self.output = nn.Conv1d(out_channels[-1], self.latent_dim, kernel_size=(1,))

    def features(self, x: T) -> T:
        assert x.ndim == 3
        n_frames = x.size(-1) // self.hop_len + 1
        with torch.no_grad():
            spec = self.spectrogram.log_power(x, n_frames, self.eps)
        y, t_out = self.tcn.forward_planes(spec, n_frames)
        return y[:, :, :t_out]

    def forward(self, x: T) -> T:
        from .cnn_generic import BinMeanHead
        f = self.features(x)                                        # (B, C, T'): Conv1d(C, L, 1) + sigmoid = the bin-mean head at one bin
        y, _ = BinMeanHead.apply(f.unsqueeze(2), self.output.weight, self.output.bias)
        return y


class SpectralDSTCN(nn.Module):
    """models.py:218-289: the strided (down-sampling) variant: TCN with stride 2 per block -> mean over time ->
    Linear(96, 48) -> PReLU -> Linear(48, latent_dim) -> sigmoid; (B, 1, N) -> (B, latent_dim)."""

    def __init__(self, n_samples: int = 88200, n_fft: int = 1024, hop_len: int = 256, kernel_size: int = 13,
                 out_channels: Optional[List[int]] = None, dilations: Optional[List[int]] = None,
                 strides: Optional[List[int]] = None, n_fc_units: int = 48, latent_dim: int = 2, use_ln: bool = True,
                 use_res: bool = True, eps: float = 1e-7) -> None:
        super().__init__()
        from .tcn import TCN
        self.n_fft, self.hop_len, self.kernel_size, self.n_fc_units, self.latent_dim = n_fft, hop_len, kernel_size, n_fc_units, latent_dim
        self.use_ln, self.use_res, self.eps = use_ln, use_res, eps
        if out_channels is None:
            out_channels = [96] * 5
        self.out_channels = out_channels
        if dilations is None:
            dilations = [2 ** idx for idx in range(len(out_channels))]
        self.dilations = dilations
        if strides is None:
            strides = [2] * len(out_channels)
        self.strides = strides
        self.spectrogram = SpectrogramHIP(n_fft, hop_len)
        self.n_frames = n_samples // hop_len + 1
        temporal_dims, cur = [self.n_frames], self.n_frames
        for stride in strides[:-1]:
            cur = math.ceil(cur / stride)
            temporal_dims.append(cur)
        self.tcn = TCN(out_channels, dilations, n_fft // 2 + 1, kernel_size, strides, padding=None, use_ln=use_ln,
                       temporal_dims=temporal_dims, use_res=use_res, is_causal=False)
        self.fc = nn.Linear(out_channels[-1], self.n_fc_units)
        self.fc_act = nn.PReLU(self.n_fc_units)
        self.output = nn.Linear(self.n_fc_units, self.latent_dim)

    def forward(self, x: T) -> T:
        assert x.ndim == 3
        n_frames = x.size(-1) // self.hop_len + 1
        with torch.no_grad():
            spec = self.spectrogram.log_power(x, n_frames, self.eps)
        y, t_out = self.tcn.forward_planes(spec, n_frames)
        from .cnn_generic import BinMeanHead, LinearPReLU, time_mean
        f = time_mean(y[:, :, :t_out])                              # models.py:283: mean over the remaining frames
        hid = LinearPReLU.apply(f, self.fc.weight, self.fc.bias, self.fc_act.weight)
        out, _ = BinMeanHead.apply(hid.view(hid.size(0), -1, 1, 1), self.output.weight, self.output.bias)   # Linear + sigmoid
        return out.view(out.size(0), -1)


class HiddenStateModel(nn.Module):
    """models.py:292-308."""

    def __init__(self) -> None:
        super().__init__()
        self.hidden: Tuple[T, T] = (torch.zeros((1,)), torch.zeros((1,)))
        self.is_hidden_init = False

    def update_hidden(self, hidden: Tuple[T, T]) -> None:
        self.hidden = hidden
        self.is_hidden_init = True

    def detach_hidden(self) -> None:
        if self.is_hidden_init:
            self.hidden = tuple((h.detach().clone() for h in self.hidden))

    def clear_hidden(self) -> None:
        self.is_hidden_init = False


LSTM_NPARAM = 17473        # 256*2 + 256*64 + 256 + 256 + 64 + 1 (csrc/lstm.hip)


def _rows(t: T) -> Tuple[int, int]:
    """(device pointer, row stride) of a (B,1,T)/(B,T) fp32 view whose rows are contiguous."""
    if not t.is_cuda:
        raise _hip.HipLibraryError("mod_extraction_amd ops need tensors on a HIP device (no CPU fallback)")
    if t.ndim == 3:
        assert t.size(1) == 1
        t = t[:, 0, :]
    assert t.dtype == torch.float32 and t.ndim == 2 and t.stride(1) == 1
    return t.data_ptr(), t.stride(0)


class LSTMEffectModel(HiddenStateModel):
    """models.py:311-339.  ``self.lstm`` / ``self.fc`` hold the parameters under the reference's
    state-dict keys (the 7 shipped ``models/lstm_64__*.pt`` files load with strict=True); the recurrence
    runs in ``mx_lstm_fwd`` (one workgroup per clip, weights in registers, state in LDS)."""

    def __init__(self, in_ch: int = 1, out_ch: int = 1, n_hidden: int = 64, latent_dim: int = 1) -> None:
        super().__init__()
        # the fused kernels of csrc/lstm.hip are the shipped LSTM-64 with one audio and one LFO channel; any other size runs
        # the general recurrence of csrc/lstm_generic.hip as an autograd node (lstm_generic.GenericLSTM)
        self.generic = (in_ch, out_ch, n_hidden, latent_dim) != (1, 1, 64, 1)
        if self.generic and not (out_ch == in_ch or out_ch == 1 or in_ch == 1):
            raise ValueError("LSTMEffectModel: fc output (out_ch) and x (in_ch) do not broadcast (models.py:338)")
        self.in_ch, self.out_ch, self.n_hidden, self.latent_dim = in_ch, out_ch, n_hidden, latent_dim
        self.lstm = nn.LSTM(in_ch + latent_dim, n_hidden, batch_first=True)     # parameter holder
        self.fc = nn.Linear(n_hidden, out_ch)                                    # parameter holder

    def _params(self) -> List[T]:
        return [self.lstm.weight_ih_l0, self.lstm.weight_hh_l0, self.lstm.bias_ih_l0, self.lstm.bias_hh_l0,
                self.fc.weight, self.fc.bias]

    def _state(self, B: int, device) -> Tuple[T, T]:
        if self.is_hidden_init:
            h, c = self.hidden
            return h.reshape(B, self.n_hidden), c.reshape(B, self.n_hidden)
        return (torch.zeros((B, self.n_hidden), device=device, dtype=torch.float32),
                torch.zeros((B, self.n_hidden), device=device, dtype=torch.float32))

    def detach_hidden(self) -> None:
        """models.py:303-305 clones the detached state; the state tensors here never carry a graph and the kernels never
        write to a state they were given as input (``mx_lstm_fwd`` writes the new state to fresh buffers), so there is
        nothing to copy."""

    def run_chunk(self, x: T, latent: T, stash: Optional[T] = None) -> Tuple[T, T, T]:
        """Forward one chunk without autograd.  Returns (y (B,1,T), h_start, c_start); updates the hidden
        state.  ``stash`` (B,T,384) receives the per-step activations when a BPTT step follows."""
        assert x.ndim == 3 and latent.shape == (x.size(0), self.latent_dim, x.size(-1))
        B, _, Tn = x.shape
        h0, c0 = self._state(B, x.device)
        h1 = torch.empty((B, 64), device=x.device, dtype=torch.float32)
        c1 = torch.empty((B, 64), device=x.device, dtype=torch.float32)
        y = torch.empty((B, 1, Tn), device=x.device, dtype=torch.float32)
        xp, xs = _rows(x)
        lp, ls = _rows(latent)
        yp, ys = _rows(y)
        w = [p.detach().contiguous() for p in self._params()]
        _hip.call("mx_lstm_fwd", xp, xs, lp, ls, _hip.ptr(w[0]), _hip.ptr(w[1]), _hip.ptr(w[2]), _hip.ptr(w[3]),
                  _hip.ptr(w[4]), _hip.ptr(w[5]), _hip.ptr(h0.contiguous()), _hip.ptr(c0.contiguous()), _hip.ptr(h1), _hip.ptr(c1),
                  yp, ys, _hip.ptr(stash), B, Tn, _hip.stream())
        self.update_hidden((h1.view(1, B, 64), c1.view(1, B, 64)))
        return y, h0, c0

    def bptt_l1_chunk(self, x: T, latent: T, y: T, wet: T, stash: T, h0: T, c0: T, loss_scale: float,
                      grad_out: Optional[T]) -> Optional[T]:
        """BPTT of one chunk with the L1 loss fused; the summed parameter gradient (17473,) in
        state-dict order is written to ``grad_out``.  ``grad_out=None``: the per-clip gradient rows (B, 17473) are returned
        unsummed (``FlatAdamW.step_from_rows`` sums them and steps in one launch)."""
        B, _, Tn = x.shape
        assert grad_out is None or (grad_out.numel() == LSTM_NPARAM and grad_out.is_contiguous())     # every element is overwritten below
        part = torch.empty((B, LSTM_NPARAM), device=x.device, dtype=torch.float32)
        xp, xs = _rows(x)
        lp, ls = _rows(latent)
        yp, ys = _rows(y)
        wp, ws = _rows(wet)
        _hip.call("mx_lstm_bwd_l1", xp, xs, lp, ls, yp, ys, wp, ws, _hip.ptr(stash),
                  _hip.ptr(self.lstm.weight_hh_l0.detach().contiguous()), _hip.ptr(self.fc.weight.detach().contiguous()),
                  _hip.ptr(h0.contiguous()), _hip.ptr(c0.contiguous()), float(loss_scale), _hip.ptr(part), B, Tn, _hip.stream())
        if grad_out is None:
            return part
        _hip.call("mx_reduce_rows", _hip.ptr(part), B, LSTM_NPARAM, 0, _hip.ptr(grad_out), _hip.stream())
        return None

    def bptt_chunk(self, x: T, latent: T, y: T, dy: T, stash: T, h0: T, c0: T, grad_out: T) -> None:
        """BPTT of one chunk for ANY loss: ``dy`` (B,1,T) or (B,T) = d loss / d y (``effect_losses.effect_loss_grad``);
        the summed parameter gradient (17473,) in state-dict order is written to ``grad_out``."""
        B, _, Tn = x.shape
        assert grad_out.numel() == LSTM_NPARAM and grad_out.is_contiguous()
        dy = dy.view(B, Tn)
        assert dy.stride(1) == 1
        part = torch.empty((B, LSTM_NPARAM), device=x.device, dtype=torch.float32)
        xp, xs = _rows(x)
        lp, ls = _rows(latent)
        yp, ys = _rows(y)
        _hip.call("mx_lstm_bwd", xp, xs, lp, ls, yp, ys, dy.data_ptr(), dy.stride(0), _hip.ptr(stash),
                  _hip.ptr(self.lstm.weight_hh_l0.detach().contiguous()), _hip.ptr(self.fc.weight.detach().contiguous()),
                  _hip.ptr(h0.contiguous()), _hip.ptr(c0.contiguous()), _hip.ptr(part), B, Tn, _hip.stream())
        _hip.call("mx_reduce_rows", _hip.ptr(part), B, LSTM_NPARAM, 0, _hip.ptr(grad_out), _hip.stream())

    def bptt_chunk_dlfo(self, x: T, latent: T, y: T, stash: T, h0: T, c0: T, grad_out: T, wet: Optional[T] = None,
                        loss_scale: float = 0.0, dy: Optional[T] = None) -> T:
        """``bptt_l1_chunk`` (``wet`` + ``loss_scale``) or ``bptt_chunk`` (``dy``) that also returns d loss / d latent (B,1,T):
        the gradient an UNFROZEN LFO model receives through the LFO it produced (lightning.py:258,361).  The kernel leaves the
        gate gradients (B,T,256); ``mx_lstm_dlfo`` contracts them with the LFO column of ``weight_ih_l0``."""
        B, _, Tn = x.shape
        assert grad_out.numel() == LSTM_NPARAM and grad_out.is_contiguous()
        assert (wet is None) != (dy is None)
        part = torch.empty((B, LSTM_NPARAM), device=x.device, dtype=torch.float32)
        dgate = torch.empty((B, Tn, 256), device=x.device, dtype=torch.float32)
        dlat = torch.empty((B, 1, Tn), device=x.device, dtype=torch.float32)
        xp, xs = _rows(x)
        lp, ls = _rows(latent)
        yp, ys = _rows(y)
        wp, ws = _rows(wet) if wet is not None else (None, 0)
        if dy is not None:
            dy = dy.view(B, Tn)
            assert dy.stride(1) == 1
        _hip.call("mx_lstm_bwd_dgate", xp, xs, lp, ls, yp, ys, wp, ws, None if dy is None else dy.data_ptr(),
                  0 if dy is None else dy.stride(0), _hip.ptr(stash), _hip.ptr(self.lstm.weight_hh_l0.detach().contiguous()),
                  _hip.ptr(self.fc.weight.detach().contiguous()), _hip.ptr(h0.contiguous()), _hip.ptr(c0.contiguous()),
                  float(loss_scale), _hip.ptr(part), _hip.ptr(dgate), B, Tn, _hip.stream())
        _hip.call("mx_reduce_rows", _hip.ptr(part), B, LSTM_NPARAM, 0, _hip.ptr(grad_out), _hip.stream())
        _hip.call("mx_lstm_dlfo", _hip.ptr(dgate), _hip.ptr(self.lstm.weight_ih_l0.detach().contiguous()), B, Tn,
                  _hip.ptr(dlat), Tn, _hip.stream())
        return dlat

    def forward(self, x: T, latent: T) -> T:
        """Inference / validation forward (no autograd graph; training goes through the fused TBPTT
        step of ``lightning.TBPTTLFOEffectModeling``).  A model of another size (``self.generic``) is an ordinary autograd node:
        gradients reach its parameters and ``latent``; the carried state is a constant (detached, as lightning.py:353,383 do)."""
        if self.generic:
            from .lstm_generic import GenericLSTM
            assert x.ndim == 3 and latent.shape == (x.size(0), self.latent_dim, x.size(-1)) and x.size(1) == self.in_ch
            B = x.size(0)
            h0, c0 = self._state(B, x.device)
            y, h1, c1 = GenericLSTM.apply(x, latent, h0, c0, *self._params())
            self.update_hidden((h1.view(1, B, self.n_hidden), c1.view(1, B, self.n_hidden)))
            return y
        with torch.no_grad():
            y, _, _ = self.run_chunk(x.contiguous().float(), latent.contiguous().float())
        return y

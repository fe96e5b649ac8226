"""Sample-rate conversion on the device (K24; csrc/resample_abi.h has the definition): recordings made at another rate than the
training rate -- most interfaces and most public dry / wet sets are at 48 kHz -- are converted once, into a cache on disk, and
the file-backed datasets then read the converted tree.

``resample_plan`` / ``resample_rows`` are the band-limited rational resampler (a Kaiser-windowed sinc, polyphase, fp64
accumulation, deterministic); ``convert_tree`` converts a directory of wav files with it.  There is no CPU path.
"""
import ctypes
import json
import logging
import os
import shutil
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor as T

from . import _hip

log = logging.getLogger(__name__)

ROUTES = ("lds", "l2")                  # MX_RESAMPLE_ROUTE_LDS, MX_RESAMPLE_ROUTE_L2
OUT_TILE = _hip.RESAMPLE_OUT_TILE
STAMP_SUFFIX = ".resampled.json"


def _int(v, name: str, fn: str) -> int:
    if isinstance(v, bool) or not isinstance(v, int):
        raise ValueError(f"{fn}: {name} must be an int, got {v!r}")
    return v


def _lib_plan(fn: str, sr_in: int, sr_out: int, zeros: int, rolloff: float, beta: float, n_in: int):
    """(up, down, half, n_out, table_floats, route) of ``mx_resample_plan``; its refusals as ValueErrors."""
    i32 = (ctypes.c_int32 * 4)()
    i64 = (ctypes.c_int64 * 2)()
    a32, a64 = ctypes.addressof(i32), ctypes.addressof(i64)
    rc = _hip.load().mx_resample_plan(sr_in, sr_out, zeros, rolloff, beta, n_in, a32, a32 + 4, a32 + 8, a64, a64 + 8, a32 + 12)
    if rc == -2:
        raise ValueError(f"{fn}: {sr_in} -> {sr_out} Hz with zeros = {zeros}, rolloff = {rolloff}, beta = {beta} on {n_in} "
                         "samples is beyond the resampler's limits (up, down <= 4096, at most 4095 taps a phase, a table of at "
                         "most 2^24 floats, beta <= 64, n up < 2^62)")
    if rc != 0:
        raise ValueError(f"{fn}: need sr_in, sr_out, zeros, n >= 1, 0 < rolloff <= 1 and beta >= 0; got {sr_in} -> {sr_out} Hz, "
                         f"zeros = {zeros}, rolloff = {rolloff}, beta = {beta}, n = {n_in}")
    return i32[0], i32[1], i32[2], i64[0], i64[1], i32[3]


class ResamplePlan:
    """What a conversion ``sr_in -> sr_out`` needs besides the samples: ``up`` / ``down`` (the rates over their gcd), ``half``
    and ``taps_per_phase`` = 2 half + 1 of the filter, ``route`` ("lds": the tap table is staged in LDS, "l2": it is read
    through L2), ``out_length(n)``, and one cached (up, taps_per_phase) fp32 tap table per device (``taps``)."""

    def __init__(self, sr_in: int, sr_out: int, zeros: int = 48, rolloff: float = 0.95, beta: float = 16.0) -> None:
        fn = "resample_plan"
        self.sr_in, self.sr_out = _int(sr_in, "sr_in", fn), _int(sr_out, "sr_out", fn)
        self.zeros, self.rolloff, self.beta = _int(zeros, "zeros", fn), float(rolloff), float(beta)
        self.up, self.down, self.half, _, self.table_floats, route = _lib_plan(fn, self.sr_in, self.sr_out, self.zeros,
                                                                               self.rolloff, self.beta, 1)
        self.taps_per_phase = 2 * self.half + 1
        self.route = ROUTES[route]
        self._tables: Dict[torch.device, T] = {}

    def out_length(self, n: int) -> int:
        """ceil(n up / down), by the library's arithmetic (a ValueError beyond its limits)."""
        fn = "ResamplePlan.out_length"
        return _lib_plan(fn, self.sr_in, self.sr_out, self.zeros, self.rolloff, self.beta, _int(n, "n", fn))[3]

    def taps(self, device) -> T:
        """The (up, taps_per_phase) fp32 tap table on ``device``: one ``mx_resample_taps`` launch the first time."""
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("ResamplePlan.taps: the table lives on a HIP device (there is no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        table = self._tables.get(device)
        if table is None:
            table = torch.empty((self.up, self.taps_per_phase), device=device, dtype=torch.float32)
            with torch.cuda.device(device):
                _hip.call("mx_resample_taps", self.up, self.down, self.half, self.rolloff, self.beta, _hip.ptr(table),
                          _hip.stream())
            self._tables[device] = table
        return table

    def __repr__(self) -> str:
        return (f"ResamplePlan({self.sr_in} -> {self.sr_out} Hz: up = {self.up}, down = {self.down}, half = {self.half}, "
                f"route = {self.route})")


def resample_plan(sr_in: int, sr_out: int, zeros: int = 48, rolloff: float = 0.95, beta: float = 16.0) -> ResamplePlan:
    """The plan of ``sr_in -> sr_out`` (positive ints).  ``zeros``: zero crossings of the sinc on each side at the cut-off
    ``rolloff`` times the lower of the two Nyquist frequencies; ``beta``: the Kaiser window's.  Host arithmetic of the library
    (``mx_resample_plan``); the tap table is built on first use."""
    return ResamplePlan(sr_in, sr_out, zeros, rolloff, beta)


def resample_rows(x: T, sr_in: int, sr_out: int, plan: Optional[ResamplePlan] = None, out: Optional[T] = None) -> T:
    """``x`` (B, n) or (n,), fp32 on the device, at ``sr_in`` -> (B, n_out) or (n_out,) at ``sr_out``, n_out =
    ceil(n up / down), in one ``mx_resample_rows`` launch per 65535 rows and without a host synchronisation.  Rows any row
    stride apart (inner stride 1) are read in place; ``out``: an fp32 tensor of the result's shape on the same device, inner
    stride 1, any row stride (a strided view is written in place; it must not share memory with ``x``).  ``plan`` defaults to
    ``resample_plan(sr_in, sr_out)``; pass one to choose the filter and to reuse its tap table.  Equal rates return
    ``x.clone()`` (or fill ``out``) without a launch of this library."""
    fn = "resample_rows"
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.ndim not in (1, 2):
        raise ValueError(f"{fn}: x must be an fp32 tensor of shape (B, n) or (n,)")
    if not x.is_cuda:
        raise ValueError(f"{fn}: x must be on a HIP device (there is no CPU fallback)")
    sr_in, sr_out = _int(sr_in, "sr_in", fn), _int(sr_out, "sr_out", fn)
    if sr_in < 1 or sr_out < 1:
        raise ValueError(f"{fn}: rates must be positive, got {sr_in} -> {sr_out}")
    if plan is None:
        plan = resample_plan(sr_in, sr_out)
    elif not isinstance(plan, ResamplePlan) or (plan.sr_in, plan.sr_out) != (sr_in, sr_out):
        raise ValueError(f"{fn}: plan is {plan!r}, not a ResamplePlan of {sr_in} -> {sr_out} Hz")
    xd = x.detach()
    rows = xd if xd.ndim == 2 else xd.unsqueeze(0)
    B, n = rows.shape
    if B < 1 or n < 1:
        raise ValueError(f"{fn}: need at least one row of at least one sample, got {tuple(x.shape)}")
    if rows.stride(1) != 1 and n > 1:
        raise ValueError(f"{fn}: the samples of a row must be contiguous (inner stride 1), got strides {tuple(x.stride())}")
    x_stride = rows.stride(0) if B > 1 else n
    if x_stride < n:
        raise ValueError(f"{fn}: rows of x overlap (row stride {x_stride} < n = {n})")
    n_out = n if sr_in == sr_out else plan.out_length(n)
    shape = (B, n_out) if x.ndim == 2 else (n_out,)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != shape or out.device != x.device:
        raise ValueError(f"{fn}: out must be an fp32 tensor of shape {shape} on x's device")
    orows = out.detach() if out.ndim == 2 else out.detach().unsqueeze(0)
    if orows.stride(1) != 1 and n_out > 1:
        raise ValueError(f"{fn}: the samples of a row of out must be contiguous (inner stride 1), got strides {tuple(out.stride())}")
    y_stride = orows.stride(0) if B > 1 else n_out
    if y_stride < n_out:
        raise ValueError(f"{fn}: rows of out overlap (row stride {y_stride} < n_out = {n_out})")
    if sr_in == sr_out:
        out.copy_(x.detach())
        return out
    with torch.cuda.device(x.device):
        table = plan.taps(x.device)
        _hip.call("mx_resample_rows", rows.data_ptr(), x_stride, B, n, plan.up, plan.down, plan.half, _hip.ptr(table),
                  orows.data_ptr(), y_stride, n_out, _hip.stream())
    return out


# ---- a directory of recordings ------------------------------------------------------------------------------------------
def _stamp_of(src: str, sr: int, plan_key: Tuple) -> Dict[str, object]:
    st = os.stat(src)
    return {"src_size": st.st_size, "src_mtime_ns": st.st_mtime_ns, "sr": sr, "filter": list(plan_key)}


def _read_stamp(path: str) -> Optional[Dict[str, object]]:
    try:
        with open(path) as f:
            return json.load(f)
    except (OSError, ValueError):
        return None


def _replace_into(dst: str, write) -> None:
    """``write(tmp)`` and then ``os.replace(tmp, dst)``: a reader never sees half a file, and processes racing on one ``dst``
    each rename a complete one."""
    tmp = f"{dst}.tmp{os.getpid()}"
    try:
        write(tmp)
        os.replace(tmp, dst)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def convert_tree(src_dir: str, dst_dir: str, sr: int, ext: str = "wav", device="cuda", zeros: int = 48, rolloff: float = 0.95,
                 beta: float = 16.0) -> Dict[str, Tuple[int, int, int]]:
    """Every ``*ext`` file under ``src_dir`` at rate ``sr`` under the same relative path in ``dst_dir``:
    ``{source path: (sr_in, frames_in, frames_out)}``.

    A file at another rate is converted on ``device`` (all its channels as the rows of one ``resample_rows`` call) and written
    as a float32 RIFF by ``datasets.wav_save``; a file already at ``sr`` is copied byte for byte.  Either way the file appears
    under its name by ``os.replace`` of a temporary one, and a stamp ``<file>.resampled.json`` beside it records the source's
    size and mtime, the rate and the filter: a file whose stamp still matches is skipped.  The conversion is deterministic, so
    the ranks of a distributed run that race on one file write the same bytes."""
    from . import datasets
    fn = "convert_tree"
    sr = _int(sr, "sr", fn)
    if sr < 1:
        raise ValueError(f"{fn}: sr must be positive, got {sr}")
    if os.path.abspath(src_dir) == os.path.abspath(dst_dir):
        raise ValueError(f"{fn}: dst_dir must differ from src_dir ({src_dir})")
    key = (int(zeros), float(rolloff), float(beta))
    plans: Dict[int, ResamplePlan] = {}
    done: Dict[str, Tuple[int, int, int]] = {}
    n_conv = n_copy = 0
    for src in datasets.list_files(src_dir, ext):
        dst = os.path.join(dst_dir, os.path.relpath(src, src_dir))
        frames, sr_in, _ = datasets.wav_info(src)
        stamp = dict(_stamp_of(src, sr, key), sr_in=sr_in, frames_in=frames)
        old = _read_stamp(dst + STAMP_SUFFIX)
        if old is not None and os.path.isfile(dst) and all(old.get(k) == v for k, v in stamp.items()):
            done[src] = (sr_in, frames, int(old["frames_out"]))
            continue
        os.makedirs(os.path.dirname(dst) or ".", exist_ok=True)
        if sr_in == sr:
            frames_out = frames
            _replace_into(dst, lambda tmp: shutil.copyfile(src, tmp))
            n_copy += 1
        else:
            if sr_in not in plans:
                plans[sr_in] = resample_plan(sr_in, sr, *key)
            audio, _ = datasets.wav_load(src)                   # (channels, frames) fp32 on the host
            y = resample_rows(audio.to(device), sr_in, sr, plan=plans[sr_in]).cpu()
            frames_out = int(y.shape[1])
            _replace_into(dst, lambda tmp: datasets.wav_save(tmp, y, sr))
            n_conv += 1
        stamp["frames_out"] = frames_out

        def write_stamp(tmp: str) -> None:
            with open(tmp, "w") as f:
                json.dump(stamp, f, sort_keys=True)

        _replace_into(dst + STAMP_SUFFIX, write_stamp)
        done[src] = (sr_in, frames, frames_out)
    log.info("%s -> %s at %d Hz: %d converted, %d copied, %d already there", src_dir, dst_dir, sr, n_conv, n_copy,
             len(done) - n_conv - n_copy)
    return done

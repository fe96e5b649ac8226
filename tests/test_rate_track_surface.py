"""CPU: the surface of the rate contour (K25) -- the declarations of mod_extraction_amd/csrc/rate_track_abi.h against
``_hip.SIGNATURES_RATE``, the limits of the four ``mx_rate_track_*`` entry points (checked before any launch, so without a
device), a stale library, ``rate_track.rate_track_plan`` against ``mx_rate_track_plan``, the Python ValueErrors, and the switches
of ``score_pair`` / ``scripts/eval_pairs.py`` being off by default.  No device work."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from tests.helpers import rate_track64 as r

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mod_extraction_amd", "csrc")
ABI_H = os.path.join(CSRC, "rate_track_abi.h")
ARG, UNSUPPORTED = -1, -2
NAMES = ["mx_rate_track_plan", "mx_rate_track_nodes", "mx_rate_track_path", "mx_rate_track_refine"]


def declared():
    """name -> parameter count of every ``int mx_*(...);`` of the header, read with this test's own regex."""
    text = re.sub(r"/\*.*?\*/", " ", open(ABI_H).read(), flags=re.S)
    return {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"^int\s+(mx_\w+)\s*\(([^;]*)\)\s*;", text, flags=re.M)}


def test_header_table_and_symbols():
    from mod_extraction_amd import _hip, build
    lib = ctypes.CDLL(build.build(verbose=False))
    counts = declared()
    assert list(counts) == list(_hip.SIGNATURES_RATE) == NAMES
    assert counts == {"mx_rate_track_plan": 15, "mx_rate_track_nodes": 18, "mx_rate_track_path": 24, "mx_rate_track_refine": 25}
    others = (_hip.SIGNATURES, _hip.SIGNATURES_TRACK, _hip.SIGNATURES_RESAMPLE)
    assert all(n.startswith("mx_rate_track_") and not any(n in t for t in others) for n in counts)
    # the other three tables and the ABI number did not move
    assert len(_hip.SIGNATURES) == 124 and _hip.ABI_VERSION == 21 == lib.mx_abi_version()
    assert list(_hip.SIGNATURES_TRACK) == ["mx_track_fit_plan", "mx_track_fit"]
    assert all(n.startswith("mx_resample_") for n in _hip.SIGNATURES_RESAMPLE) and len(_hip.SIGNATURES_RESAMPLE) >= 1
    bound = _hip.load()
    zeros = {ctypes.c_void_p: None, ctypes.c_int64: 0, ctypes.c_int32: 0, ctypes.c_float: 0.0, ctypes.c_double: 0.0}
    for name, n_args in counts.items():
        assert hasattr(lib, name) and len(_hip.SIGNATURES_RATE[name]) == n_args
        fn = getattr(bound, name)
        assert fn.argtypes == _hip.SIGNATURES_RATE[name] and fn.restype is ctypes.c_int      # load() binds the fourth table
        assert fn(*[zeros[t] for t in _hip.SIGNATURES_RATE[name]]) == ARG                    # all-zero arguments are refused
    assert '#include "rate_track_abi.h"' in open(os.path.join(CSRC, "rate_track.hip")).read()
    assert "rate_track_abi" not in open(os.path.join(CSRC, "common.h")).read()
    lim = {k: int(v) for k, v in re.findall(r"#define\s+MX_RATE_TRACK_(\w+)\s+(\d+)\s*$", open(ABI_H).read(), flags=re.M)}
    assert lim == _hip.RATE_TRACK_LIMITS == {"MIN_W": 16, "MAX_W": 4096, "MAX_S": 16384, "MAX_STATES": 8192, "MAX_D": 16,
                                             "MAX_N": 1 << 20, "MAX_ROWS": 65535, "CAND_TILE": 256}


DEFAULTS = dict(B=2, n=2760, sr=172.5, S=16, W=345, f_min=0.25, f_max=8.0, mask=0x3F, rate_div=4, J=32, L=4, D=2, stride=None,
                rw=0.002, pw=1.0, node_bytes=1 << 50, ws_bytes=1 << 50, null=(), node=16, ws=16)


def _p(kw, name, value=16):
    return None if name in kw["null"] else ctypes.c_void_p(value)


def plan(**over):
    """(status, K, node_bytes, ws_bytes) of ``mx_rate_track_plan``; ``null``: which of its three host outputs are missing."""
    from mod_extraction_amd import _hip
    kw = dict(DEFAULTS, **over)
    sizes = (ctypes.c_int64 * 3)(-7, -7, -7)
    a = ctypes.addressof(sizes)
    rc = _hip.load().mx_rate_track_plan(kw["B"], kw["n"], kw["sr"], kw["S"], kw["W"], kw["f_min"], kw["f_max"], kw["mask"],
                                        kw["rate_div"], kw["J"], kw["L"], kw["D"], None if "K" in kw["null"] else a,
                                        None if "node_bytes" in kw["null"] else a + 8, None if "ws_bytes" in kw["null"] else a + 16)
    return rc, sizes[0], sizes[1], sizes[2]


def nodes(**over):
    """``mx_rate_track_nodes`` on pointers that are never read: EVERY call of this, ``path`` and ``refine`` below is one the
    library refuses before a launch (only ``plan``, which is host arithmetic, is also called with arguments it accepts)."""
    from mod_extraction_amd import _hip
    kw = dict(DEFAULTS, **over)
    return _hip.load().mx_rate_track_nodes(_p(kw, "y"), kw["n"] if kw["stride"] is None else kw["stride"], kw["B"], kw["n"], kw["sr"],
                                           _p(kw, "starts"), kw["S"], kw["W"], kw["f_min"], kw["f_max"], kw["mask"], kw["rate_div"],
                                           kw["J"], _p(kw, "node", kw["node"]), kw["node_bytes"], _p(kw, "ws", kw["ws"]),
                                           kw["ws_bytes"], None)


def path(**over):
    from mod_extraction_amd import _hip
    kw = dict(DEFAULTS, **over)
    outs = [_p(kw, k) for k in ("shape", "grid_k", "grid_j", "cost", "per_shape_cost")]
    return _hip.load().mx_rate_track_path(kw["B"], kw["n"], kw["sr"], _p(kw, "starts"), kw["S"], kw["W"], kw["f_min"], kw["f_max"],
                                          kw["mask"], kw["rate_div"], kw["J"], kw["D"], kw["rw"], kw["pw"],
                                          _p(kw, "node", kw["node"]), kw["node_bytes"], _p(kw, "ws", kw["ws"]), kw["ws_bytes"], *outs,
                                          None)


def refine(**over):
    from mod_extraction_amd import _hip
    kw = dict(DEFAULTS, **over)
    ptrs = [_p(kw, k) for k in ("shape", "grid_k", "grid_j", "rate_hz", "phase", "amp", "offset", "resid")]
    return _hip.load().mx_rate_track_refine(_p(kw, "y"), kw["n"] if kw["stride"] is None else kw["stride"], kw["B"], kw["n"],
                                            kw["sr"], _p(kw, "starts"), kw["S"], kw["W"], kw["f_min"], kw["f_max"], kw["mask"],
                                            kw["rate_div"], kw["J"], kw["L"], *ptrs, _p(kw, "ws", kw["ws"]), kw["ws_bytes"], None)


def test_limits_are_checked_before_any_launch():
    everyone = (lambda **kw: plan(**kw)[0], nodes, path, refine)
    for call in everyone:
        assert call(B=0) == ARG and call(B=-3) == ARG
        assert call(f_min=0.0) == ARG and call(f_min=-1.0) == ARG and call(f_min=3.0, f_max=2.0) == ARG
        assert call(f_max=86.25) == ARG and call(f_max=100.0) == ARG and call(f_min=float("nan")) == ARG
        assert call(mask=0) == ARG and call(mask=0x80) == ARG
        assert call(W=15, n=2760) == UNSUPPORTED and call(W=4097, n=8000) == UNSUPPORTED
        assert call(S=0) == UNSUPPORTED and call(S=16385) == UNSUPPORTED
        assert call(J=3) == UNSUPPORTED and call(J=129) == UNSUPPORTED
        assert call(rate_div=0) == UNSUPPORTED and call(rate_div=17) == UNSUPPORTED
        assert call(n=(1 << 20) + 1) == UNSUPPORTED and call(B=65536) == UNSUPPORTED
        assert call(n=344) == ARG                                             # a row shorter than one slice
        assert call(J=128, f_max=8.25) == UNSUPPORTED                         # K = 65 at W = 345: 65 x 128 states > 8192
        # K18's order: a bad window before a bad size
        assert call(W=15, f_min=0.0) == ARG
    assert plan(J=128, f_max=8.0)[:2] == (0, 63) and plan(J=128, f_max=8.125)[:2] == (0, 64)       # 8192 states
    assert plan(J=128, f_max=8.25)[0] == UNSUPPORTED                                                 # 65 x 128
    assert plan(W=690, n=10350, S=29)[:2] == (0, 125) and plan(D=16)[0] == 0 and plan(D=0, L=0, S=16384, n=1 << 20)[0] == 0
    for call in (lambda **kw: plan(**kw)[0], path):
        assert call(D=-1) == UNSUPPORTED and call(D=17) == UNSUPPORTED
    for call in (lambda **kw: plan(**kw)[0], refine):
        assert call(L=-1) == ARG and call(L=9) == UNSUPPORTED
    # pointers: among the first
    for name in ("y", "starts", "node", "ws"):
        assert nodes(null=(name,)) == ARG, name
    for name in ("starts", "node", "ws", "shape", "grid_k", "grid_j", "cost", "per_shape_cost"):
        assert path(null=(name,)) == ARG, name
    for name in ("y", "starts", "shape", "grid_k", "grid_j", "rate_hz", "phase", "amp", "offset", "resid", "ws"):
        assert refine(null=(name,)) == ARG, name
    for name in ("K", "node_bytes", "ws_bytes"):
        assert plan(null=(name,)) == (ARG, -7, -7, -7), name                  # a refused plan writes nothing
    assert plan(W=15)[1:] == (-7, -7, -7)
    # a short stride where K18 checks it: after the sizes, before the grid
    assert nodes(stride=2759) == ARG and refine(stride=2759) == ARG and nodes(stride=3, W=15) == UNSUPPORTED
    assert nodes(stride=2759, J=128, f_max=8.25) == ARG
    # the weights
    for bad in (-1.0, float("nan"), float("inf")):
        assert path(rw=bad) == ARG and path(pw=bad) == ARG
    # the buffers: 16-byte aligned and at least what the plan reports
    rc, K, node_bytes, ws_bytes = plan()
    assert (rc, K) == (0, 63) and node_bytes == 8 * 2 * 7 * 16 * 63 * 32
    assert ws_bytes == 8 * (2 * 2 * 16 + 2 * 2 * 7) + 4 * 2 * 7 * 16 * 63 * 32 and ws_bytes % 16 == 0
    for call in (nodes, path):
        assert call(node_bytes=node_bytes - 1) == ARG and call(ws_bytes=ws_bytes - 1) == ARG
        assert call(node=24) == ARG and call(ws=24) == ARG
    assert refine(ws_bytes=ws_bytes - 1) == ARG and refine(ws=24) == ARG


def test_a_stale_library_names_the_fourth_header(monkeypatch):
    from mod_extraction_amd import _hip, build
    build.build(verbose=False)
    monkeypatch.setattr(_hip, "_lib", None)
    monkeypatch.setattr(_hip, "SIGNATURES_RATE", dict(_hip.SIGNATURES_RATE, mx_rate_track_of_tomorrow=[ctypes.c_void_p]))
    with pytest.raises(_hip.HipLibraryError,
                       match=r"mx_rate_track_of_tomorrow.*csrc/rate_track_abi\.h.*rebuild.*python -m mod_extraction_amd\.build"):
        _hip.load()
    monkeypatch.undo()
    assert _hip.load() is not None


# (n, sr, slice, hop, window, rate_div, n_phases)
PLAN_TABLE = [
    (10350, 172.5, 690, 345, (0.25, 8.0), 4, 32),                    # the 60 s track at the defaults: S = 29, K = 125
    (2760, 172.5, 345, 172, (0.25, 4.0), 4, 32),
    (689, 172.5, 345, 172, (0.25, 8.125), 4, 4),
    (150, 31.5, 64, 64, (1.0, 1.0), 4, 8),                           # K = 1
    (72, 8.0, 16, 7, (0.25, 2.0), 4, 32),
    (101, 31.5, 64, None, (0.25, 6.0), 1, 128),
    (103500, 172.4987, 690, 345, (0.1, 7.3), 3, 32),                 # ten minutes; values that are no fp32 numbers
    (4096, 172.5, 4096, None, (0.5, 0.6), 16, 4),                    # one slice, the longest
]


def test_rate_track_plan_against_the_library():
    from mod_extraction_amd import rate_track as R
    for n, sr, W, hop, window, rate_div, J in PLAN_TABLE:
        S, K = R.rate_track_plan(n, sr, W, hop, window, rate_div, J)
        assert S == len(r.window_starts(n, W, W // 2 if hop is None else hop))
        assert K == r.grid(W, sr, window[0], window[1], rate_div)[4]
        rc, k_lib, node_bytes, _ = plan(B=1, n=n, sr=sr, S=S, W=W, f_min=window[0], f_max=window[1], rate_div=rate_div, J=J)
        assert (rc, k_lib, node_bytes) == (0, K, 8 * 7 * S * K * J), (n, W)
    assert R.rate_track_plan(10350, 172.5, 690, 345) == (29, 125)
    assert inspect.signature(R.fit_rate_track).parameters["max_rate_step"].default == 2
    defaults = {k: v.default for k, v in inspect.signature(R.fit_rate_track).parameters.items()}
    assert (defaults["rate_div"], defaults["n_phases"], defaults["n_rounds"], defaults["rate_weight"], defaults["phase_weight"],
            defaults["rate_hz"], defaults["hop_points"]) == (4, 32, 4, 0.002, 1.0, (0.25, 8.0), None)
    for bad in (dict(slice_points=15), dict(slice_points=4097, n=9000), dict(n=300), dict(n=(1 << 20) + 1), dict(rate_div=0),
                dict(rate_div=17), dict(n_phases=3), dict(n_phases=129), dict(hop_points=0), dict(hop_points=346),
                dict(rate_hz=(0.0, 8.0)), dict(rate_hz=(0.25, 8.25), n_phases=128), dict(n=20000, slice_points=16, hop_points=1),
                dict(slice_points=345.0)):
        with pytest.raises(ValueError, match="fit_rate_track|fit_lfo"):
            R.rate_track_plan(**dict(dict(n=2760, sr=172.5, slice_points=345), **bad))


def test_value_errors_come_before_any_launch(monkeypatch):
    from mod_extraction_amd import _hip, rate_track as R
    calls = []
    monkeypatch.setattr(_hip, "call", lambda name, *a: calls.append(name))
    with pytest.raises(ValueError, match="HIP device"):
        R.fit_rate_track(torch.zeros(2, 2760), 172.5, 345)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    y = torch.zeros(2, 2760)
    for kw in (dict(n_rounds=9), dict(n_rounds=-1), dict(max_rate_step=17), dict(max_rate_step=-1), dict(rate_weight=-1.0),
               dict(phase_weight=float("nan")), dict(shapes=()), dict(shapes=("sine",)), dict(n_phases=3), dict(slice_points=15),
               dict(hop_points=400), dict(rate_hz=(0.25, 90.0))):
        with pytest.raises(ValueError):
            R.fit_rate_track(y, 172.5, **dict(dict(slice_points=345), **kw))
    with pytest.raises(ValueError):
        R.fit_rate_track(torch.zeros(2, 2760, dtype=torch.float64), 172.5, 345)
    with pytest.raises(ValueError):
        R.fit_rate_track(torch.zeros(0, 2760), 172.5, 345)
    assert calls == []


def test_the_switches_default_to_off():
    from mod_extraction_amd import file_eval
    assert inspect.signature(file_eval.score_pair).parameters["rate_track"].default is None
    text = open(os.path.join(ROOT, "scripts", "eval_pairs.py")).read()
    m = re.search(r'add_argument\("--rate_track",\s*default=None', text)
    assert m is not None and "rate_track=rate_track" in text

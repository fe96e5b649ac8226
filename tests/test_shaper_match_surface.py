"""CPU: the surface of the shaper match (K27) -- the declarations of mod_extraction_amd/csrc/shaper_match_abi.h against
``_hip.SIGNATURES_SHAPER`` with the other five tables untouched, the argument checks and limits of the six entry points (all
before any launch, in the documented order, so without a device), those of ``shaper.py``, a stale library, the step's new
arguments, exclusion rules and metric names, and the shipped config.  No device work."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

from tests.helpers import shaper_match64 as h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mod_extraction_amd", "csrc")
ABI_H = os.path.join(CSRC, "shaper_match_abi.h")
ARG, UNSUPPORTED = -1, -2
COUNTS = {"mx_shaper_match_partials": 10, "mx_shaper_match_solve": 13, "mx_shaper_match_apply": 12,
          "mx_shaper_match_bwd_partials": 11, "mx_shaper_match_bwd_solve": 10, "mx_shaper_match_bwd_apply": 18}


def declared():
    """name -> parameter count of every ``int mx_*(...);`` of the header, read with this test's own regex."""
    text = re.sub(r"/\*.*?\*/", " ", open(ABI_H).read(), flags=re.S)
    return {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"^int\s+(mx_\w+)\s*\(([^;]*)\)\s*;", text, flags=re.M)}


def test_header_table_and_symbols():
    from mod_extraction_amd import _hip, build, shaper
    lib = ctypes.CDLL(build.build(verbose=False))
    counts = declared()
    assert counts == COUNTS and list(counts) == list(_hip.SIGNATURES_SHAPER) == list(COUNTS)
    others = (_hip.SIGNATURES, _hip.SIGNATURES_TRACK, _hip.SIGNATURES_RESAMPLE, _hip.SIGNATURES_RATE, _hip.SIGNATURES_WARP)
    assert not any(n in t for n in counts for t in others)
    # the other five tables and the ABI number did not move
    assert len(_hip.SIGNATURES) == 124 and _hip.ABI_VERSION == 21 == lib.mx_abi_version()
    assert list(_hip.SIGNATURES_TRACK) == ["mx_track_fit_plan", "mx_track_fit"]
    assert list(_hip.SIGNATURES_RESAMPLE) == ["mx_resample_plan", "mx_resample_taps", "mx_resample_rows"]
    assert list(_hip.SIGNATURES_RATE) == ["mx_rate_track_plan", "mx_rate_track_nodes", "mx_rate_track_path", "mx_rate_track_refine"]
    assert list(_hip.SIGNATURES_WARP) == ["mx_warp_plan", "mx_warp_rows"]
    text = open(os.path.join(ROOT, "include", "modex_hip.h")).read()
    assert "mx_shaper" not in text and "MX_SHAPER" not in text and "shaper_match_abi" not in text
    assert _hip.parse_signatures(text) == _hip.SIGNATURES
    bound = _hip.load()
    zeros = {ctypes.c_void_p: None, ctypes.c_int64: 0, ctypes.c_int32: 0, ctypes.c_float: 0.0, ctypes.c_double: 0.0}
    for name, n_args in counts.items():
        assert hasattr(lib, name) and len(_hip.SIGNATURES_SHAPER[name]) == n_args
        fn = getattr(bound, name)
        assert fn.argtypes == _hip.SIGNATURES_SHAPER[name] and fn.restype is ctypes.c_int     # load() binds the sixth table
        assert fn(*[zeros[t] for t in _hip.SIGNATURES_SHAPER[name]]) == ARG                   # all-zero arguments are refused
    src = open(os.path.join(CSRC, "shaper_match.hip")).read()
    assert '#include "shaper_match_abi.h"' in src and '#include "rows_common.h"' in src
    assert "shaper_match_abi" not in open(os.path.join(CSRC, "common.h")).read()
    define = lambda name: re.search(rf"#define\s+{name}\s+(\S+)", open(ABI_H).read()).group(1)
    assert int(define("MX_SHAPER_CHUNK")) == h.CHUNK == _hip.SHAPER_CHUNK == shaper.CHUNK == 2048
    assert int(define("MX_SHAPER_MAX_ORDER")) == h.MAX_ORDER == shaper.MAX_ORDER == 7
    assert int(define("MX_SHAPER_MAX_N")) == 1 << 24 and int(define("MX_SHAPER_MAX_ROWS")) == 65535


def test_a_stale_library_names_the_sixth_header(monkeypatch):
    from mod_extraction_amd import _hip, build
    build.build(verbose=False)
    monkeypatch.setattr(_hip, "_lib", None)
    monkeypatch.setattr(_hip, "SIGNATURES_SHAPER", dict(_hip.SIGNATURES_SHAPER, mx_shaper_of_tomorrow=[ctypes.c_void_p]))
    with pytest.raises(_hip.HipLibraryError,
                       match=r"mx_shaper_of_tomorrow.*csrc/shaper_match_abi\.h.*rebuild.*python -m mod_extraction_amd\.build"):
        _hip.load()
    monkeypatch.undo()
    assert _hip.load() is not None


def test_powers_and_layout():
    from mod_extraction_amd import shaper
    assert shaper.powers(5) == (1, 3, 5) == h.powers(5) and shaper.powers(4) == (1, 3) and shaper.powers(1, True) == (1,)
    assert shaper.powers(7, True) == (1, 2, 3, 4, 5, 6, 7) and shaper.powers(6, True) == h.powers(6, True)
    for order in range(1, 8):
        for even in (False, True):
            assert shaper.n_sums(order, even) == h.n_sums(order, even)
    assert shaper.n_sums(7, True) == 1 + 13 + 7 + 1 and shaper.n_sums(7) == 1 + 7 + 4 + 1 and shaper.n_sums(1) == 4
    assert h.moment_orders(5) == (2, 4, 6, 8, 10) and h.moment_orders(3, True) == (2, 3, 4, 5, 6)
    assert shaper.n_chunks(2048) == 1 and shaper.n_chunks(2049) == 2


X, Y, Z, W = 1 << 30, 1 << 31, 1 << 32, 1 << 40       # pointers that are never read: every case below is refused before a launch
P = lambda v: None if v is None else ctypes.c_void_p(v)


def lib():
    from mod_extraction_amd import _hip
    return _hip.load()


def partials(x=X, xs=1000, y=Y, ys=1000, B=2, N=1000, order=5, even=0, ws=W):
    return lib().mx_shaper_match_partials(P(x), xs, P(y), ys, B, N, order, even, P(ws), None)


def solve(ws=W, B=2, N=1000, nc=1, order=5, even=0, ridge=1e-9, max_gain=20.0, c=X, r=Y, s=Z, f=Z + (1 << 20)):
    return lib().mx_shaper_match_solve(P(ws), B, N, nc, order, even, ridge, max_gain, P(c), P(r), P(s), P(f), None)


def apply(x=X, xs=1000, c=W, r=W + 4096, f=W + 8192, B=2, N=1000, order=5, even=0, z=Y, zs=1000):
    return lib().mx_shaper_match_apply(P(x), xs, P(c), P(r), P(f), B, N, order, even, P(z), zs, None)


def bwd_partials(d=X, ds=1000, x=Y, xs=1000, r=Z, B=2, N=1000, order=5, even=0, ws=W):
    return lib().mx_shaper_match_bwd_partials(P(d), ds, P(x), xs, P(r), B, N, order, even, P(ws), None)


def bwd_solve(ws=W, s=X, f=Y, B=2, nc=1, order=5, even=0, ridge=1e-9, u=Z):
    return lib().mx_shaper_match_bwd_solve(P(ws), P(s), P(f), B, nc, order, even, ridge, P(u), None)


def bwd_apply(d=X, ds=1000, x=Y, xs=1000, y=Z, ys=1000, c=W, r=W + 4096, u=W + 8192, f=W + 12288, B=2, N=1000, order=5, even=0,
              ridge=1e-9, o=X + (1 << 20), os_=1000):
    return lib().mx_shaper_match_bwd_apply(P(d), ds, P(x), xs, P(y), ys, P(c), P(r), P(u), P(f), B, N, order, even, ridge, P(o),
                                           os_, None)


def test_entry_point_checks_before_any_launch():
    nan, big = float("nan"), (1 << 24) + 1
    # NULL pointers, shapes and strides
    assert partials(x=None) == partials(y=None) == partials(ws=None) == partials(B=0) == partials(N=0) == partials(xs=999) == ARG
    assert partials(ys=999) == ARG
    assert solve(ws=None) == solve(c=None) == solve(r=None) == solve(s=None) == solve(f=None) == solve(B=0) == solve(N=0) == ARG
    assert solve(nc=2) == ARG and solve(N=2049, nc=1) == ARG and solve(N=2049, nc=3) == ARG    # n_chunks is ceil(N / 2048)
    assert apply(x=None) == apply(c=None) == apply(r=None) == apply(f=None) == apply(z=None) == apply(zs=999) == ARG
    assert bwd_partials(d=None) == bwd_partials(x=None) == bwd_partials(r=None) == bwd_partials(ws=None) == bwd_partials(ds=1) == ARG
    assert bwd_solve(ws=None) == bwd_solve(s=None) == bwd_solve(f=None) == bwd_solve(u=None) == bwd_solve(B=0) == bwd_solve(nc=0) == ARG
    assert bwd_apply(d=None) == bwd_apply(y=None) == bwd_apply(c=None) == bwd_apply(u=None) == bwd_apply(o=None) == ARG
    assert bwd_apply(os_=999) == ARG
    # the order and the switch
    for fn in (partials, solve, apply, bwd_partials, bwd_solve, bwd_apply):
        assert fn(order=0) == fn(order=8) == fn(even=2) == fn(even=-1) == ARG
    # ridge and max_gain
    assert solve(ridge=-1e-12) == solve(ridge=nan) == solve(ridge=math.inf) == solve(max_gain=0.5) == solve(max_gain=nan) == ARG
    assert bwd_solve(ridge=-1.0) == bwd_solve(ridge=nan) == bwd_apply(ridge=-1.0) == bwd_apply(ridge=math.inf) == ARG
    # limits: after the arguments, before the overlaps
    assert partials(N=big, xs=big, ys=big) == partials(B=65536) == UNSUPPORTED
    assert solve(N=big, nc=8193) == solve(B=65536) == UNSUPPORTED
    assert apply(N=big, xs=big, zs=big) == bwd_partials(N=big, ds=big, xs=big) == UNSUPPORTED
    assert bwd_apply(N=big, ds=big, xs=big, ys=big, os_=big) == bwd_solve(B=65536) == bwd_solve(nc=8193) == UNSUPPORTED
    assert partials(N=big, xs=big, ys=big, order=0) == ARG and solve(B=65536, ridge=-1.0) == ARG         # an argument before a limit
    assert apply(N=big, xs=big, zs=big, z=X) == UNSUPPORTED                                                 # a limit before an overlap
    # overlaps: an output shares a byte with an input or with another output
    assert partials(ws=X + 4 * 1999) == ARG and partials(ws=Y - 8) == ARG and partials(ws=X - 8) == ARG
    assert solve(c=W) == solve(r=W + 8) == solve(s=W) == solve(f=W + 16) == ARG and solve(r=X + 4) == solve(f=Z + 8) == ARG
    assert apply(z=X + 4 * 1999) == apply(z=X - 4 * 1999) == apply(z=W - 4 * 1999) == apply(z=W + 4096) == apply(z=W + 8192 + 4) == ARG
    assert bwd_partials(ws=X) == bwd_partials(ws=Y + 4) == bwd_partials(ws=Z - 8) == ARG
    assert bwd_solve(u=W) == bwd_solve(u=X + 8) == bwd_solve(u=Y - 8) == ARG
    assert bwd_apply(o=Y) == bwd_apply(o=Z + 4) == bwd_apply(o=W) == bwd_apply(o=W + 8192) == bwd_apply(o=W + 12288 + 4) == ARG
    assert bwd_apply(o=X + 4) == ARG and bwd_apply(o=X, os_=1001) == ARG      # dz itself only with dz's stride


def test_python_checks_in_their_order():
    """``match_shaper`` / ``match_shaper_backward`` on CPU tensors: the arguments are refused before the tensors are looked
    at, the tensors' shapes before the device is asked for, and the LAST refusal is the device's."""
    from mod_extraction_amd import shaper as S
    x = torch.zeros(2, 100)
    for bad in (0, 8, 2.0, True, "3", None):
        with pytest.raises(ValueError, match="order must be an integer in 1 .. 7"):
            S.match_shaper(x.double(), x, order=bad, even=1, ridge=-1.0)
    with pytest.raises(ValueError, match="even must be True or False"):
        S.match_shaper(x.double(), x, even=1, ridge=-1.0)
    for bad in (-1e-12, math.nan, math.inf, "0", True):
        with pytest.raises(ValueError, match="ridge must be a finite number >= 0"):
            S.match_shaper(x.double(), x, ridge=bad, max_gain=0.0)
    for bad in (0.99, math.nan, math.inf, None):
        with pytest.raises(ValueError, match="max_gain must be a finite number >= 1"):
            S.match_shaper(x.double(), x, max_gain=bad)
    with pytest.raises(ValueError, match="y_hat must be an fp32 tensor"):
        S.match_shaper(x.double(), x)
    with pytest.raises(ValueError, match="HIP device"):
        S.match_shaper(x, x)
    m = S.ShaperMatch(x, torch.zeros(2, 3), torch.zeros(2), torch.zeros(2, S.n_sums(5), dtype=torch.float64),
                      torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="match must be the ShaperMatch"):
        S.match_shaper_backward(x, x, x, (x,), False, 1e-9)
    with pytest.raises(ValueError, match="match.coeffs must be"):
        S.match_shaper_backward(x, x, x, m._replace(coeffs=torch.zeros(2, 8)), False, 1e-9)
    with pytest.raises(ValueError, match="even must be the forward's"):
        S.match_shaper_backward(x, x, x, m, 0, 1e-9)
    with pytest.raises(ValueError, match="ridge must be"):
        S.match_shaper_backward(x, x, x, m, False, -1.0)
    with pytest.raises(ValueError, match="HIP device"):
        S.match_shaper_backward(x, x, x, m, False, 1e-9)
    assert [p.name for p in inspect.signature(S.match_shaper_backward).parameters.values() if p.default is inspect.Parameter.empty] \
        == ["dz", "y_hat", "y", "match", "even", "ridge"]                      # the forward's values: no defaults
    sig = inspect.signature(S.match_shaper).parameters
    assert {k: v.default for k, v in sig.items() if v.default is not inspect.Parameter.empty} \
        == {"order": 5, "even": False, "ridge": 1e-9, "max_gain": 20.0, "out": None}
    mod = S.MatchShaper()
    assert (mod.order, mod.even, mod.ridge, mod.max_gain, mod.last) == (5, False, 1e-9, 20.0, None) and list(mod.parameters()) == []
    with pytest.raises(ValueError, match="MatchShaper: order"):
        S.MatchShaper(order=9)


def mk(**kw):
    from mod_extraction_amd import lightning
    return lightning.LFOExtractionThroughEffect(torch.nn.Identity(), **kw)


def test_step_arguments_and_metric_names(monkeypatch):
    from mod_extraction_amd import _hip, file_eval, lightning
    calls = []
    monkeypatch.setattr(_hip, "call", lambda name, *a: calls.append(name))
    names = list(inspect.signature(lightning.LFOExtractionThroughEffect.__init__).parameters)
    assert names[-4:] == ["match_shaper", "match_shaper_even", "match_shaper_ridge", "match_shaper_max_gain"]   # appended
    plain = mk()
    assert (plain.match_shaper, plain.match_shaper_even, plain.match_shaper_ridge, plain.match_shaper_max_gain) == (None, False, 1e-9, 20.0)
    assert plain.step_metric_names == [] and plain._shaper is None and not plain._matched
    # validated at construction even when off
    for kw, msg in (({"match_shaper": 0}, "order must be"), ({"match_shaper": 8}, "order must be"), ({"match_shaper": 3.0}, "order"),
                    ({"match_shaper_even": 1}, "even must be"), ({"match_shaper_ridge": -1.0}, "ridge must be"),
                    ({"match_shaper_max_gain": 0.5}, "max_gain must be"), ({"match_shaper": 5, "match_shaper_ridge": math.nan}, "ridge")):
        with pytest.raises(ValueError, match="match_shaper: " + msg):
            mk(**kw)
    shaper_names = ["shaper/linear", "shaper/curve", "shaper/flagged"]
    assert mk(match_shaper=5).step_metric_names == shaper_names
    assert mk(match_shaper=3, match_gain="ls").step_metric_names == ["gain/mean", "gain/std", "gain/clamped"] + shaper_names
    assert mk(match_shaper=7, match_shaper_even=True, match_fir=9).step_metric_names == ["fir/dc_gain", "fir/l1", "fir/flagged"] + shaper_names
    assert mk(match_fir=9).step_metric_names == ["fir/dc_gain", "fir/l1", "fir/flagged"] and mk(match_gain="rms")._matched
    with pytest.raises(ValueError, match="mutually exclusive"):                 # the two linear matches still exclude each other
        mk(match_gain="ls", match_fir=9, match_shaper=5)
    for kw in ({"match_shaper": 5}, {"match_shaper": 5, "match_fir": 9, "warmup_ms": 110}):
        step = mk(**kw)
        assert list(step.state_dict()) == list(plain.state_dict()) and list(step.parameters()) == [] and list(step.buffers()) == []
        assert [n for n, _ in step.named_modules()] == [n for n, _ in plain.named_modules()] and step.loss_dict == plain.loss_dict
    assert list(inspect.signature(file_eval.score_pair).parameters)[-1] == "drift"
    assert calls == []


def test_shipped_config():
    """train_lfo_pairs_flanger_shaper.yml is train_lfo_pairs_flanger_fir.yml plus ``match_shaper: 5``."""
    import yaml
    from mod_extraction_amd import cli, lightning
    load = lambda name: yaml.safe_load(open(os.path.join(ROOT, "configs", name)))
    new, base = load("train_lfo_pairs_flanger_shaper.yml"), load("train_lfo_pairs_flanger_fir.yml")
    assert new["model"]["init_args"].pop("match_shaper") == 5
    assert new == base
    old = os.getcwd()
    os.chdir(os.path.join(ROOT, "scripts"))
    try:
        c = cli.CustomLightningCLI(args=["fit", "-c", "../configs/train_lfo_pairs_flanger_shaper.yml"], run=False, device=torch.device("cpu"))
    finally:
        os.chdir(old)
    assert isinstance(c.model, lightning.LFOExtractionThroughEffect) and c.model.match_fir == 9 and c.model.match_shaper == 5
    assert not c.model.match_shaper_even and c.model.match_shaper_ridge == 1e-9 and c.model.match_shaper_max_gain == 20.0
    assert c.model.step_metric_names[-3:] == ["shaper/linear", "shaper/curve", "shaper/flagged"]

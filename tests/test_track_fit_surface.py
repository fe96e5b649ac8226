"""CPU: the surface of the track fit (K23) -- the declarations of mod_extraction_amd/csrc/track_fit_abi.h against
``_hip.SIGNATURES_TRACK``, the limits of ``mx_track_fit`` / ``mx_track_fit_plan`` (checked before any launch, so without a
device), a stale library, and ``modulations.fit_plan`` against tests/helpers/lfo_fit64.grid_of.  No device work."""
import ctypes
import os
import re

import pytest
import torch

from tests.helpers import lfo_fit64 as h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI_H = os.path.join(ROOT, "mod_extraction_amd", "csrc", "track_fit_abi.h")
ARG, UNSUPPORTED = -1, -2


def declared():
    """name -> parameter count of every ``int mx_*(...);`` of the header, read with this test's own regex."""
    text = re.sub(r"/\*.*?\*/", " ", open(ABI_H).read(), flags=re.S)
    return {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"^int\s+(mx_\w+)\s*\(([^;]*)\)\s*;", text, flags=re.M)}


def test_header_table_and_symbols():
    from mod_extraction_amd import _hip, build, modulations as M
    lib = ctypes.CDLL(build.build(verbose=False))
    counts = declared()
    assert list(counts) == list(_hip.SIGNATURES_TRACK) == ["mx_track_fit_plan", "mx_track_fit"]
    assert counts == {"mx_track_fit_plan": 11, "mx_track_fit": 21}
    assert all(n.startswith("mx_track_fit") and n not in _hip.SIGNATURES for n in counts)
    assert len(_hip.SIGNATURES) == 124 and _hip.ABI_VERSION == 21 == lib.mx_abi_version()      # the first table did not move
    bound = _hip.load()
    for name, n_args in counts.items():
        assert hasattr(lib, name) and len(_hip.SIGNATURES_TRACK[name]) == n_args
        fn = getattr(bound, name)
        assert fn.argtypes == _hip.SIGNATURES_TRACK[name] and fn.restype is ctypes.c_int     # load() binds the second table
        zeros = {ctypes.c_void_p: None, ctypes.c_int64: 0, ctypes.c_int32: 0, ctypes.c_float: 0.0}
        assert fn(*[zeros[t] for t in _hip.SIGNATURES_TRACK[name]]) == ARG
    # the definitions are compiled against the declarations, and common.h stays with the one public header
    csrc = os.path.join(ROOT, "mod_extraction_amd", "csrc")
    assert '#include "track_fit_abi.h"' in open(os.path.join(csrc, "track_fit.hip")).read()
    assert "track_fit_abi" not in open(os.path.join(csrc, "common.h")).read()
    tile = int(re.search(r"#define\s+MX_TRACK_FIT_ROW_TILE\s+(\d+)", open(ABI_H).read()).group(1))
    assert M.TRACK_FIT_ROW_TILE == _hip.TRACK_FIT_ROW_TILE == tile and tile >= 64


def fit(B=4, n=345, sr=172.5, f_min=0.25, f_max=8.0, mask=0x3F, rate_div=4, J=32, L=4, y=16, stride=None, out=16, table=None,
        ws=16, ws_bytes=1 << 40):
    """``mx_track_fit`` on pointers that are never read: every case below is refused before a launch."""
    from mod_extraction_amd import _hip
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    outs = [p(out)] * 6 if not isinstance(out, (list, tuple)) else [p(v) for v in out]
    return _hip.load().mx_track_fit(p(y), n if stride is None else stride, B, n, sr, f_min, f_max, mask, rate_div, J, L, *outs,
                                    p(table), p(ws), ws_bytes, None)


def plan(B=4, n=345, sr=172.5, f_min=0.25, f_max=8.0, mask=0x3F, rate_div=4, J=32, L=4, null=()):
    """(status, K, ws_bytes) of ``mx_track_fit_plan``; ``null``: which of its two host outputs are missing."""
    from mod_extraction_amd import _hip
    sizes = (ctypes.c_int64 * 2)(-7, -7)
    a = ctypes.addressof(sizes)
    rc = _hip.load().mx_track_fit_plan(B, n, sr, f_min, f_max, mask, rate_div, J, L, None if "K" in null else a,
                                       None if "ws" in null else a + 8)
    return rc, sizes[0], sizes[1]


def test_limits_are_checked_before_any_launch():
    for call in (fit, lambda **kw: plan(**kw)[0]):
        assert call(B=0) == ARG and call(B=-3) == ARG
        assert call(f_min=0.0) == ARG and call(f_min=-1.0) == ARG and call(f_min=3.0, f_max=2.0) == ARG
        assert call(f_max=86.25) == ARG and call(f_max=100.0) == ARG and call(f_min=float("nan")) == ARG
        assert call(mask=0) == ARG and call(mask=0x80) == ARG and call(L=-1) == ARG
        assert call(n=15) == UNSUPPORTED and call(n=0) == UNSUPPORTED and call(n=(1 << 20) + 1, f_max=0.3) == UNSUPPORTED
        assert call(J=3) == UNSUPPORTED and call(J=129) == UNSUPPORTED and call(L=9) == UNSUPPORTED
        assert call(rate_div=0) == UNSUPPORTED and call(rate_div=17) == UNSUPPORTED
        # 2^20 points at 65536 Hz and rate_div 16 have df = 2^-8: 1 .. 4097 - 2^-8 Hz is K = 2^20 and one df more is 2^20 + 1
        assert call(n=1 << 20, sr=65536.0, f_min=1.0, f_max=4097.0, rate_div=16) == UNSUPPORTED
    assert fit(y=None) == ARG and fit(ws=None) == ARG and fit(stride=344) == ARG
    for k in range(6):                                                       # every output vector is required
        assert fit(out=[None if i == k else 16 for i in range(6)]) == ARG, k
    assert plan(null=("K",))[0] == ARG and plan(null=("ws",))[0] == ARG
    # K18's order: a bad window before a bad size, a bad size before a short stride, a short stride before the grid
    assert fit(n=15, f_min=0.0) == ARG and fit(n=15, stride=3) == UNSUPPORTED
    assert fit(n=1 << 20, sr=65536.0, f_min=1.0, f_max=4097.0, rate_div=16, stride=5) == ARG
    # the workspace: 16-byte aligned and at least what the plan reports
    rc, K, ws_bytes = plan()
    assert rc == 0 and K == h.grid_of(345, 172.5, 0.25, 8.0, 4)[4] == 63
    tiles = -(-K * 32 // 256)
    assert ws_bytes == 4 * (7 * tiles * 16 + 8 * (345 + 2 + 21))
    assert fit(ws_bytes=ws_bytes - 1) == ARG and fit(ws=24) == ARG
    assert plan(n=1 << 20, sr=65536.0, f_min=1.0, f_max=4097.0 - 2.0 ** -8, rate_div=16)[:2] == (0, 1 << 20)
    assert plan(null=("K",))[1:] == (-7, -7) and plan(n=15)[1:] == (-7, -7)          # a refused plan writes nothing


def test_a_stale_library_names_the_second_header(monkeypatch):
    from mod_extraction_amd import _hip, build
    build.build(verbose=False)
    monkeypatch.setattr(_hip, "_lib", None)
    monkeypatch.setattr(_hip, "SIGNATURES_TRACK", dict(_hip.SIGNATURES_TRACK, mx_track_fit_of_tomorrow=[ctypes.c_void_p]))
    with pytest.raises(_hip.HipLibraryError,
                       match=r"mx_track_fit_of_tomorrow.*csrc/track_fit_abi\.h.*rebuild.*python -m mod_extraction_amd\.build"):
        _hip.load()
    monkeypatch.undo()
    assert _hip.load() is not None


# (n, sr, window, rate_div) -> the route; K is the helper's
PLAN_TABLE = [
    ((345, 172.5, (0.25, 8.0), 4), "lfo_fit"),
    ((4096, 172.5, (0.5, 0.6), 4), "lfo_fit"),
    ((4097, 172.5, (0.5, 0.6), 4), "track_fit"),                     # one point more than K18 takes
    ((345, 172.5, (0.25, 16.21875), 16), "lfo_fit"),                 # K = 512
    ((345, 172.5, (0.25, 16.25), 16), "track_fit"),                  # K = 513
    ((4096, 172.5, (0.25, 8.0), 4), "track_fit"),                    # K = 737 on a row K18 would take
    ((4097, 172.5, (0.5, 2.0), 4), "track_fit"),
    ((10350, 172.5, (0.25, 8.0), 4), "track_fit"),
    ((16, 8.0, (0.25, 2.0), 4), "lfo_fit"),
    ((63, 31.5, (0.25, 6.0), 1), "lfo_fit"),
    ((1035, 172.4987, (0.1, 7.3), 3), "lfo_fit"),                    # values that are no fp32 numbers
]


def test_fit_plan_against_the_helper():
    from mod_extraction_amd import modulations as M
    ks = {}
    for (n, sr, window, rate_div), route in PLAN_TABLE:
        K = h.grid_of(n, sr, window[0], window[1], rate_div)[4]
        assert M.fit_plan(n, sr, window, rate_div) == (route, K), (n, sr, window, rate_div)
        assert route == ("lfo_fit" if n <= 4096 and K <= 512 else "track_fit")
        rc, k_lib, _ = plan(B=1, n=n, sr=sr, f_min=window[0], f_max=window[1], rate_div=rate_div)
        assert (rc, k_lib) == (0, K)                                          # the library's K: one formula
        ks[(n, window[1], rate_div)] = K
    assert ks[(345, 16.21875, 16)] == 512 and ks[(345, 16.25, 16)] == 513 and ks[(4096, 8.0, 4)] == 737
    assert ks[(4097, 2.0, 4)] == 143 and ks[(10350, 8.0, 4)] == 1861
    assert M.fit_plan(345, 172.5) == ("lfo_fit", 63)                          # the defaults
    # what has no grid goes where it went before; past the new limits it is a ValueError
    assert M.fit_plan(15, 172.5) == ("lfo_fit", 0) and M.fit_plan(345, 172.5, rate_div=0) == ("lfo_fit", 0)
    for bad in (dict(n=(1 << 20) + 1, sr=172.5), dict(n=1 << 20, sr=65536.0, rate_hz=(1.0, 4097.0), rate_div=16),
                dict(n=4097, sr=172.5, rate_div=17), dict(n=345, sr=172.5, rate_hz=(0.0, 8.0))):
        with pytest.raises(ValueError):
            M.fit_plan(**bad)
    assert M.fit_plan(1 << 20, 65536.0, (1.0, 4097.0 - 2.0 ** -8), 16) == ("track_fit", 1 << 20)


def test_new_limits_are_value_errors_before_any_launch(monkeypatch):
    """``fit_lfo`` checks the tensor first (a CPU tensor is refused: no fallback); with that check out of the way the limits
    of the new route are raised before ``_hip.call`` is reached."""
    from mod_extraction_amd import _hip, modulations as M
    calls = []
    monkeypatch.setattr(_hip, "call", lambda name, *a: calls.append(name))
    with pytest.raises(ValueError, match="HIP device"):
        M.fit_lfo(torch.zeros(2, 4097), 172.5, (0.5, 2.0))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    for kw in (dict(n_phases=3), dict(n_phases=129), dict(n_rounds=9), dict(n_rounds=-1), dict(rate_div=0), dict(rate_div=17)):
        with pytest.raises(ValueError):
            M.fit_lfo(torch.zeros(2, 4097), 172.5, (0.5, 2.0), **kw)
    with pytest.raises(ValueError, match="rates"):
        M.fit_lfo(torch.zeros(1, 1 << 20), 65536.0, (1.0, 4097.0), rate_div=16)
    with pytest.raises(ValueError, match="at most"):
        M.fit_lfo(torch.zeros(1, (1 << 20) + 1), 172.5, (0.5, 2.0))
    assert calls == []

"""CPU: the surface of the file-level tools (``mod_extraction_amd.file_eval``, K22) -- ``window_starts``, the declaration of
``mx_lfo_stitch`` in include/modex_hip.h against ``_hip.SIGNATURES``, the limits of ``mx_lfo_stitch`` (checked before any launch, so
without a device) and the wrappers' ``ValueError``s.  No device work."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = -1, -2


@pytest.mark.parametrize("N", [64, 22272, 7])
def test_window_starts(N):
    from mod_extraction_amd.file_eval import window_starts
    hops = sorted({N, max(1, N // 2), max(1, N // 4), max(1, (N * 3) // 7), 1 if N < 100 else 1000})
    for L in (N, N + 1, 3 * N + 17):
        for hop in hops:
            s = window_starts(L, N, hop)
            assert s[0] == 0 and s[-1] == L - N and len(set(s)) == len(s) and s == sorted(s)
            covered = [False] * L
            for a in s:
                assert 0 <= a <= L - N
                covered[a:a + N] = [True] * N
            assert all(covered), (L, N, hop)
            regular = [a for a in s if a % hop == 0]
            assert regular == list(range(0, L - N + 1, hop)) and len(s) - len(regular) <= 1
            assert all(b - a <= hop for a, b in zip(s, s[1:]))
        assert window_starts(L, N) == window_starts(L, N, max(1, N // 2))          # the default hop
    assert window_starts(N, N, 1) == [0] and window_starts(N + 1, N, N) == [0, 1]


def test_window_starts_errors():
    from mod_extraction_amd.file_eval import window_starts
    with pytest.raises(ValueError, match="shorter"):
        window_starts(63, 64)
    for hop in (0, -1, 65):
        with pytest.raises(ValueError, match="hop"):
            window_starts(200, 64, hop)
    for bad in (32.0, "32", True):
        with pytest.raises(ValueError, match="hop"):
            window_starts(200, 64, bad)
    with pytest.raises(ValueError, match="N must"):
        window_starts(200, 0)
    with pytest.raises(ValueError, match="L must"):
        window_starts(200.0, 64)


def test_header_table_and_symbol():
    """The one ``mx_lfo_stitch`` name, declared in include/modex_hip.h -- the one header: ``include/`` holds no other, and
    csrc/common.h includes no other -- and read here with a regex of this test's own; it is exported; the argument count and
    the bound argtypes are those of ``_hip.SIGNATURES``, which is what the parser makes of that text (ABI 21)."""
    from mod_extraction_amd import _hip, build, file_eval
    lib = ctypes.CDLL(build.build(verbose=False))
    assert [f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h")] == ["modex_hip.h"]
    raw = open(os.path.join(ROOT, "include", "modex_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    found = [(n, a) for n, a in re.findall(r"\bint\s+(mx_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S) if "stitch" in n]
    assert [n for n, _ in found] == ["mx_lfo_stitch"] == [n for n in _hip.SIGNATURES if "stitch" in n]
    params = [" ".join(a.split()) for a in found[0][1].split(",")]
    assert len(params) == 10 == len(_hip.SIGNATURES["mx_lfo_stitch"])
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    assert _hip.SIGNATURES["mx_lfo_stitch"] == [P, P, I64, I64, I64, I64, I64, P, P, P]
    assert [("*" in a) for a in params] == [t is P for t in _hip.SIGNATURES["mx_lfo_stitch"]]
    assert _hip.SIGNATURES == _hip.parse_signatures(raw) and _hip.ABI_VERSION == 21
    assert int(re.search(r"^#define MX_STITCH_MAX_WINDOWS \(1 << (\d+)\)$", raw, flags=re.M).group(1)) == 20
    assert file_eval.MAX_WINDOWS == 1 << 20
    common = open(os.path.join(ROOT, "mod_extraction_amd", "csrc", "common.h")).read()
    assert re.findall(r'#include\s+"(modex_hip\w*\.h)"', common) == ["modex_hip.h"]
    assert hasattr(lib, "mx_lfo_stitch")
    fn = _hip.load().mx_lfo_stitch
    assert fn.argtypes == _hip.SIGNATURES["mx_lfo_stitch"] and fn.restype is ctypes.c_int


def p(v):
    return None if v is None else ctypes.c_void_p(v)


A0, S0, T0, C0 = 1 << 20, 2 << 20, 3 << 20, 4 << 20


def stitch(windows=A0, starts=S0, W=5, n_f=345, N=22272, L=66833, n_t=1035, track=T0, cover=C0):
    from mod_extraction_amd import _hip
    return _hip.load().mx_lfo_stitch(p(windows), p(starts), W, n_f, N, L, n_t, p(track), p(cover), None)


def test_limits_are_checked_before_any_launch():
    """Every case is refused on pointers that are never read (a case that would launch is not tried here)."""
    from mod_extraction_amd import _hip
    fn = _hip.load().mx_lfo_stitch
    assert fn(None, None, 0, 0, 0, 0, 0, None, None, None) == ARG                       # null and zero arguments
    for name in ("windows", "starts", "track", "cover"):
        assert stitch(**{name: None}) == ARG, name
    assert stitch(W=0) == ARG and stitch(W=-1) == ARG
    assert stitch(n_f=1) == ARG and stitch(n_f=0) == ARG
    assert stitch(N=1) == ARG and stitch(N=0) == ARG
    assert stitch(L=22271) == ARG and stitch(L=0) == ARG
    assert stitch(n_t=1) == ARG and stitch(n_t=0) == ARG
    assert stitch(W=(1 << 20) + 1) == UNSUPPORTED
    assert stitch(L=(1 << 31) + 1) == UNSUPPORTED
    assert stitch(n_f=(1 << 22) + 1) == UNSUPPORTED and stitch(n_t=(1 << 22) + 1) == UNSUPPORTED
    # 5 windows of 345 floats from A0 end at A0 + 6900; 1035 outputs are 4140 bytes
    assert stitch(track=A0) == ARG and stitch(track=A0 + 6896) == ARG and stitch(cover=A0 + 4) == ARG
    assert stitch(track=S0 + 8) == ARG and stitch(cover=S0) == ARG
    assert stitch(cover=T0) == ARG and stitch(cover=T0 + 4136) == ARG and stitch(track=C0 + 4136) == ARG


def test_wrapper_errors_are_raised_before_the_launch(monkeypatch):
    from mod_extraction_amd import _hip, file_eval as F
    calls = []
    monkeypatch.setattr(_hip, "call", lambda name, *a: calls.append(name))
    x = torch.zeros(3, 5)
    with pytest.raises(ValueError, match="no CPU fallback"):
        F.stitch_lfo(x, [0, 32, 64], 128, 64)
    for bad in (x.double(), torch.zeros(5), [[0.0] * 5]):
        with pytest.raises(ValueError, match="fp32"):
            F.stitch_lfo(bad, [0], 128, 64)
    with pytest.raises(ValueError, match="fx_head"):
        F.render_file(type("S", (), {"fx_head": object()})(), torch.zeros(100), torch.zeros(10))
    with pytest.raises(ValueError, match="no CPU fallback"):
        F.extract_lfo_track(lambda t: t, torch.zeros(100), n_samples=64)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    with pytest.raises(ValueError, match="two points"):
        F.stitch_lfo(torch.zeros(3, 1), [0, 32, 64], 128, 64)
    with pytest.raises(ValueError, match="2 <= N <= L"):
        F.stitch_lfo(x, [0, 32, 64], 63, 64)
    with pytest.raises(ValueError, match="2 starts for 3"):
        F.stitch_lfo(x, [0, 32], 128, 64)
    for bad in ([0, 64, 32], [-1, 0, 1], [0, 32, 65]):
        with pytest.raises(ValueError, match="ascend"):
            F.stitch_lfo(x, bad, 128, 64)
    with pytest.raises(ValueError, match="n_t"):
        F.stitch_lfo(x, [0, 32, 64], 128, 64, n_t=1)
    with pytest.raises(ValueError, match="out must"):
        F.stitch_lfo(x, [0, 32, 64], 128, 64, n_t=10, out=torch.zeros(11))
    with pytest.raises(ValueError, match="out must"):
        F.stitch_lfo(x, [0, 32, 64], 128, 64, n_t=10, out=torch.zeros(20)[::2])
    with pytest.raises(ValueError, match="shorter"):
        F.extract_lfo_track(lambda t: t, torch.zeros(63), n_samples=64)
    with pytest.raises(ValueError, match="same length"):
        F.extract_lfo_track(lambda t: t, torch.zeros(100), torch.zeros(99), n_samples=64)
    with pytest.raises(ValueError, match=r"\(L,\) or \(1, L\)"):
        F.extract_lfo_track(lambda t: t, torch.zeros(2, 100), n_samples=64)
    assert calls == []
    assert F.default_track_points(66833, 22272, 345) == 1035 and F.default_track_points(64, 64, 2) == 2
    monkeypatch.setattr(_hip, "stream", lambda: 0)
    track, cover = F.stitch_lfo(x, [0, 32, 64], 128, 64)
    assert calls == ["mx_lfo_stitch"] and track.shape == cover.shape == (10,) and cover.dtype == torch.int32


def test_windows_are_stacked_views():
    """The mini-batches ``extract_lfo_track`` shows the model: window i is ``x[starts[i] : starts[i] + N]``, the right-aligned
    last one included, whatever the mini-batch boundaries."""
    from mod_extraction_amd import file_eval as F
    N, hop, L = 16, 6, 61
    x = torch.arange(L, dtype=torch.float32)
    starts = F.window_starts(L, N, hop)
    assert starts[-1] == L - N and starts[-1] % hop != 0
    for bs in (1, 3, len(starts), 100):
        got = torch.cat([F._windows_of(x, starts, i, min(i + bs, len(starts)), N, hop) for i in range(0, len(starts), bs)])
        assert got.shape == (len(starts), 1, N)
        assert torch.equal(got[:, 0], torch.stack([x[s:s + N] for s in starts]))

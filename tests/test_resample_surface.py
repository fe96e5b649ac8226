"""CPU: the surface of the resampler (K24) -- the declarations of mod_extraction_amd/csrc/resample_abi.h against
``_hip.SIGNATURES_RESAMPLE``, the argument checks and limits of the three entry points (all before any launch, so without a
device), a stale library, ``resample.resample_plan`` against tests/helpers/resample64.plan, the ValueErrors of
``resample_rows``, and the path and stamp logic of ``convert_tree`` with the launch replaced.  No device work."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from tests.helpers import resample64 as h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI_H = os.path.join(ROOT, "mod_extraction_amd", "csrc", "resample_abi.h")
ARG, UNSUPPORTED = -1, -2
NAMES = ["mx_resample_plan", "mx_resample_taps", "mx_resample_rows"]


def declared():
    """name -> parameter count of every ``int mx_*(...);`` of the header, read with this test's own regex."""
    text = re.sub(r"/\*.*?\*/", " ", open(ABI_H).read(), flags=re.S)
    return {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"^int\s+(mx_\w+)\s*\(([^;]*)\)\s*;", text, flags=re.M)}


def define(name):
    return re.search(rf"#define\s+{name}\s+(.+?)\s*(?:/\*|$)", open(ABI_H).read(), flags=re.M).group(1)


def test_header_table_and_symbols():
    from mod_extraction_amd import _hip, build, resample
    lib = ctypes.CDLL(build.build(verbose=False))
    counts = declared()
    assert list(counts) == list(_hip.SIGNATURES_RESAMPLE) == NAMES
    assert counts == {"mx_resample_plan": 12, "mx_resample_taps": 7, "mx_resample_rows": 12}
    assert all(n not in _hip.SIGNATURES and n not in _hip.SIGNATURES_TRACK for n in counts)
    assert len(_hip.SIGNATURES) == 124 and _hip.ABI_VERSION == 21 == lib.mx_abi_version()      # the first table did not move
    assert list(_hip.SIGNATURES_TRACK) == ["mx_track_fit_plan", "mx_track_fit"]                # nor the second
    bound = _hip.load()
    for name, n_args in counts.items():
        assert hasattr(lib, name) and len(_hip.SIGNATURES_RESAMPLE[name]) == n_args
        fn = getattr(bound, name)
        assert fn.argtypes == _hip.SIGNATURES_RESAMPLE[name] and fn.restype is ctypes.c_int   # load() binds the third table
        zeros = {ctypes.c_void_p: None, ctypes.c_int64: 0, ctypes.c_int32: 0, ctypes.c_double: 0.0}
        assert fn(*[zeros[t] for t in _hip.SIGNATURES_RESAMPLE[name]]) == ARG
    csrc = os.path.join(ROOT, "mod_extraction_amd", "csrc")
    assert '#include "resample_abi.h"' in open(os.path.join(csrc, "resample.hip")).read()
    assert '#include "rows_common.h"' in open(os.path.join(csrc, "resample.hip")).read()
    assert "resample_abi" not in open(os.path.join(csrc, "common.h")).read()
    # the limits are exported, and the helper restates the two that shape the launches
    assert define("MX_RESAMPLE_MAX_FACTOR") == "4096" and define("MX_RESAMPLE_MAX_TAPS") == "4095"
    assert define("MX_RESAMPLE_MAX_TABLE") == "(1 << 24)" and define("MX_RESAMPLE_MAX_SPAN") == "(1LL << 62)"
    assert int(define("MX_RESAMPLE_OUT_TILE")) == h.OUT_TILE == _hip.RESAMPLE_OUT_TILE == resample.OUT_TILE
    assert define("MX_RESAMPLE_LDS_TABLE_BYTES") == "(160 * 1024)" and h.LDS_TABLE_BYTES == 160 * 1024


def test_the_public_header_is_untouched():
    """include/modex_hip.h knows nothing of K24: its 124 declarations, ABI number 21, and not one of the new names."""
    from mod_extraction_amd import _hip
    text = open(os.path.join(ROOT, "include", "modex_hip.h")).read()
    assert "mx_resample" not in text and "MX_RESAMPLE" not in text and "resample_abi" not in text
    table = _hip.parse_signatures(text)
    assert len(table) == 124 and table == _hip.SIGNATURES and list(table)[-1] == list(_hip.SIGNATURES)[-1]
    assert _hip.ABI_VERSION == 21


def lib_plan(sr_in=48000, sr_out=44100, zeros=48, rolloff=0.95, beta=16.0, n_in=1000, null=None):
    """(status, up, down, half, n_out, table_floats, route) of ``mx_resample_plan``; ``null``: the index of a missing output."""
    from mod_extraction_amd import _hip
    i32, i64 = (ctypes.c_int32 * 4)(-7, -7, -7, -7), (ctypes.c_int64 * 2)(-7, -7)
    a, b = ctypes.addressof(i32), ctypes.addressof(i64)
    outs = [a, a + 4, a + 8, b, b + 8, a + 12]
    if null is not None:
        outs[null] = None
    rc = _hip.load().mx_resample_plan(sr_in, sr_out, zeros, rolloff, beta, n_in, *outs)
    return rc, i32[0], i32[1], i32[2], i64[0], i64[1], i32[3]


def lib_taps(up=147, down=160, half=55, rolloff=0.95, beta=16.0, taps=16):
    from mod_extraction_amd import _hip
    return _hip.load().mx_resample_taps(up, down, half, rolloff, beta, None if taps is None else ctypes.c_void_p(taps), None)


def lib_rows(x=1 << 20, x_stride=None, B=2, n_in=1000, up=147, down=160, half=55, taps=1 << 30, y=1 << 40, y_stride=None, n_out=None):
    """``mx_resample_rows`` on pointers that are never read: every case below is refused before a launch."""
    from mod_extraction_amd import _hip
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    n_out = -(-n_in * up // down) if n_out is None else n_out
    return _hip.load().mx_resample_rows(p(x), n_in if x_stride is None else x_stride, B, n_in, up, down, half, p(taps), p(y),
                                        n_out if y_stride is None else y_stride, n_out, None)


def test_plan_checks_and_limits():
    st = lambda **kw: lib_plan(**kw)[0]
    assert lib_plan() == (0, 147, 160, 55, 919, 147 * 111, 0)
    for k in range(6):
        assert lib_plan(null=k) == (ARG,) + (-7,) * 6                           # a refused plan writes nothing
    assert st(sr_in=0) == ARG and st(sr_out=-1) == ARG and st(zeros=0) == ARG and st(n_in=0) == ARG
    assert st(rolloff=0.0) == ARG and st(rolloff=1.01) == ARG and st(rolloff=float("nan")) == ARG
    assert st(beta=-0.1) == ARG and st(beta=float("nan")) == ARG
    assert st(beta=64.0) == 0 and st(beta=64.5) == UNSUPPORTED
    assert st(sr_in=4096, sr_out=4095) == 0
    assert st(sr_in=4097, sr_out=4096) == UNSUPPORTED and st(sr_in=4096, sr_out=4097) == UNSUPPORTED      # up, down <= 4096
    assert st(sr_in=1, sr_out=1, zeros=2047, rolloff=1.0) == 0                                          # T = 4095
    assert st(sr_in=1, sr_out=1, zeros=2048, rolloff=1.0) == UNSUPPORTED
    # up T <= 2^24 cannot be passed alone: 4096 * 4095 = 2^24 - 4096, the largest table the other two limits allow
    assert 4096 * 4095 < 1 << 24 and st(sr_in=1, sr_out=4096, zeros=2047, rolloff=1.0) == 0
    assert st(sr_in=4095, sr_out=4096, zeros=2047, rolloff=0.999) == UNSUPPORTED                         # T = 4099 > 4095
    assert st(sr_in=1, sr_out=4096, n_in=1 << 50) == UNSUPPORTED and st(sr_in=1, sr_out=1, n_in=1 << 62) == UNSUPPORTED
    # at most 2^31 - 1 tiles of 4096 outputs (which n_in up < 2^62 alone would not ensure)
    most = ((1 << 31) - 1) * 4096
    assert lib_plan(sr_in=2, sr_out=1, n_in=most * 2)[::4] == (0, most) and st(sr_in=2, sr_out=1, n_in=most * 2 + 1) == UNSUPPORTED
    assert st(zeros=0, sr_in=4097, sr_out=4096) == ARG                                                  # arguments before limits
    assert st(beta=65.0, sr_in=4097, sr_out=4096) == UNSUPPORTED
    assert lib_plan(n_in=1)[4] == 1 and lib_plan(sr_in=8, sr_out=3, n_in=9)[4] == 4


def test_taps_and_rows_checks_before_any_launch():
    assert lib_taps(taps=None) == ARG and lib_taps(up=0) == ARG and lib_taps(down=0) == ARG and lib_taps(half=0) == ARG
    assert lib_taps(up=6, down=4) == ARG                                        # not in lowest terms
    assert lib_taps(rolloff=0.0) == ARG and lib_taps(beta=-1.0) == ARG and lib_taps(beta=65.0) == UNSUPPORTED
    assert lib_taps(up=4097, down=1) == UNSUPPORTED and lib_taps(up=1, down=4097) == UNSUPPORTED
    assert lib_taps(half=2048) == UNSUPPORTED                                   # T = 4097
    assert lib_taps(up=0, half=2048) == ARG
    assert lib_rows(x=None) == ARG and lib_rows(taps=None) == ARG and lib_rows(y=None) == ARG
    assert lib_rows(B=0) == ARG and lib_rows(n_in=0, n_out=1) == ARG and lib_rows(n_out=0) == ARG
    assert lib_rows(x_stride=999) == ARG and lib_rows(y_stride=918) == ARG
    assert lib_rows(up=0, n_out=5) == ARG and lib_rows(down=0, n_out=5) == ARG and lib_rows(half=0) == ARG
    assert lib_rows(up=6, down=4) == ARG
    assert lib_rows(up=4097, down=1) == UNSUPPORTED and lib_rows(up=1, down=4097) == UNSUPPORTED and lib_rows(half=2048) == UNSUPPORTED
    assert lib_rows(up=4096, down=1, n_in=1 << 50, n_out=1 << 62) == UNSUPPORTED
    assert lib_rows(up=1, down=4096, half=2047, n_in=(1 << 62) - 1) == UNSUPPORTED         # 2^50 outputs: too many tiles
    assert lib_rows(n_out=918) == ARG and lib_rows(n_out=920) == ARG            # n_out is ceil(n_in up / down) = 919
    # order: a short stride before a limit, a limit before a wrong n_out, a wrong n_out before an overlap
    assert lib_rows(x_stride=3, up=4097, down=1) == ARG and lib_rows(up=4097, down=1, n_out=1) == UNSUPPORTED
    # y shares a byte with x, or with the table
    assert lib_rows(x=1 << 20, y=(1 << 20) + 4 * 1999) == ARG
    assert lib_rows(taps=1 << 30, y=(1 << 30) + 4 * (147 * 111 - 1)) == ARG
    assert lib_rows(taps=1 << 30, y=(1 << 30) - 4 * (919 + 918)) == ARG         # y's last float is the table's first


def test_a_stale_library_names_the_third_header(monkeypatch):
    from mod_extraction_amd import _hip, build
    build.build(verbose=False)
    monkeypatch.setattr(_hip, "_lib", None)
    monkeypatch.setattr(_hip, "SIGNATURES_RESAMPLE", dict(_hip.SIGNATURES_RESAMPLE, mx_resample_of_tomorrow=[ctypes.c_void_p]))
    with pytest.raises(_hip.HipLibraryError,
                       match=r"mx_resample_of_tomorrow.*csrc/resample_abi\.h.*rebuild.*python -m mod_extraction_amd\.build"):
        _hip.load()
    monkeypatch.undo()
    assert _hip.load() is not None


# (sr_in, sr_out) -> (up, down, half, T) by the header's formula, and the route.  The header is the law and the helper its
# restatement; the figures here are worked by hand from it: 48 -> 44.1 kHz has c = 0.95 * 147 / 160 = 0.8728125 and
# 48 / c = 54.99..., so half = ceil(54.99...) = 55 and T = 111 (55 c = 48.0047 > 48: the ceil decides it by a margin of 1e-4).
PLANS = [
    ((48000, 44100), (147, 160, 55, 111), "lds"),
    ((44100, 48000), (160, 147, 51, 103), "lds"),
    ((96000, 44100), (147, 320, 110, 221), "lds"),
    ((22050, 44100), (2, 1, 51, 103), "lds"),
    ((44100, 32000), (320, 441, 70, 141), "l2"),                    # 180 KB of taps: no LDS holds them
]


@pytest.mark.parametrize("rates, figures, route", PLANS)
def test_resample_plan_against_the_helper(rates, figures, route):
    from mod_extraction_amd import resample
    pl, want = resample.resample_plan(*rates), h.plan(*rates)
    assert (pl.up, pl.down, pl.half, pl.taps_per_phase) == want[:4] == figures
    assert pl.route == route == resample.ROUTES[want.route] and pl.table_floats == pl.up * pl.taps_per_phase
    for n in (1, 2, 159, 160, 161, 4096, 96000, 2880000):
        assert pl.out_length(n) == want.out_length(n)
    for zeros, rolloff, beta in ((32, 0.95, 12.0), (4, 0.9, 5.0), (64, 1.0, 0.0)):
        pl, want = resample.resample_plan(*rates, zeros, rolloff, beta), h.plan(*rates, zeros, rolloff, beta)
        assert (pl.up, pl.down, pl.half, pl.taps_per_phase, pl.route) == want[:4] + (resample.ROUTES[want.route],)


def test_resample_plan_value_errors():
    from mod_extraction_amd import resample
    for bad in (dict(sr_in=0, sr_out=44100), dict(sr_in=48000, sr_out=-1), dict(sr_in=48000.0, sr_out=44100),
                dict(sr_in=48000, sr_out=44100, zeros=0), dict(sr_in=48000, sr_out=44100, rolloff=1.5),
                dict(sr_in=48000, sr_out=44100, beta=-1.0), dict(sr_in=48000, sr_out=44101),     # up = 44101
                dict(sr_in=48000, sr_out=44100, zeros=4000), dict(sr_in=True, sr_out=44100)):
        with pytest.raises(ValueError, match="resample_plan"):
            resample.resample_plan(**bad)
    with pytest.raises(ValueError, match="limits"):
        resample.resample_plan(48000, 44100).out_length(1 << 60)
    with pytest.raises(ValueError, match="HIP device"):
        resample.resample_plan(48000, 44100).taps("cpu")


def test_resample_rows_value_errors(monkeypatch):
    """``resample_rows`` checks the tensor first (a CPU tensor is refused: no fallback); with that check out of the way every
    other refusal comes before ``_hip.call`` is reached."""
    from mod_extraction_amd import _hip, resample
    calls = []
    monkeypatch.setattr(_hip, "call", lambda name, *a: calls.append(name))
    x = torch.zeros(2, 1000)
    with pytest.raises(ValueError, match="HIP device"):
        resample.resample_rows(x, 48000, 44100)
    for bad in (x.double(), torch.zeros(2, 3, 4), [0.0, 1.0], torch.zeros((), dtype=torch.float32)):
        with pytest.raises(ValueError, match="fp32 tensor of shape"):
            resample.resample_rows(bad, 48000, 44100)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(resample.ResamplePlan, "taps", lambda self, device: torch.zeros(1))
    rr = resample.resample_rows
    for args, msg in (((x, 0, 44100), "positive"), ((x, 48000.0, 44100), "must be an int"), ((x, 48000, 44101), "limits"),
                      ((torch.zeros(2, 0), 48000, 44100), "at least one"), ((torch.zeros(0, 5), 48000, 44100), "at least one"),
                      ((torch.zeros(2, 2000)[:, ::2], 48000, 44100), "inner stride"),
                      ((torch.zeros(1, 1000).expand(2, 1000), 48000, 44100), "overlap")):
        with pytest.raises(ValueError, match=msg):
            rr(*args)
    with pytest.raises(ValueError, match="not a ResamplePlan of 48000 -> 44100"):
        rr(x, 48000, 44100, plan=resample.resample_plan(44100, 48000))
    with pytest.raises(ValueError, match="not a ResamplePlan"):
        rr(x, 48000, 44100, plan=(147, 160))
    for out, msg in ((torch.zeros(2, 918), "out must be"), (torch.zeros(2, 919, dtype=torch.float64), "out must be"),
                     (torch.zeros(919), "out must be"), (torch.zeros(2, 2 * 919)[:, ::2], "inner stride"),
                     (torch.zeros(1, 919).expand(2, 919), "overlap")):
        with pytest.raises(ValueError, match=msg):
            rr(x, 48000, 44100, out=out)
    assert calls == []
    # what passes the checks is one launch, with the strides of the views as they are
    args = []
    monkeypatch.setattr(_hip, "call", lambda name, *a: args.append((name,) + a))
    monkeypatch.setattr(_hip, "ptr", lambda t: 77)
    monkeypatch.setattr(_hip, "stream", lambda: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda d: __import__("contextlib").nullcontext())
    wide, out = torch.zeros(2, 1003), torch.zeros(2, 1024)
    y = rr(wide[:, 3:], 48000, 44100, out=out[:, 5:5 + 919])
    assert y.shape == (2, 919) and y.data_ptr() == out.data_ptr() + 20
    assert args == [("mx_resample_rows", wide.data_ptr() + 12, 1003, 2, 1000, 147, 160, 55, 77, out.data_ptr() + 20, 1024, 919, 0)]
    args.clear()
    one = rr(torch.zeros(1000), 48000, 44100)
    assert one.shape == (919,) and args[0][2:5] == (1000, 1, 1000) and args[0][10:12] == (919, 919)
    # equal rates: a copy, no launch
    args.clear()
    src = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    same = rr(src, 44100, 44100)
    assert args == [] and torch.equal(same, src) and same.data_ptr() != src.data_ptr()


def _write_wav(path, sr, data):
    from scipy.io import wavfile
    os.makedirs(os.path.dirname(path), exist_ok=True)
    wavfile.write(path, sr, data)


def test_convert_tree_paths_and_stamps(tmp_path, monkeypatch):
    from mod_extraction_amd import datasets, resample
    src, dst = str(tmp_path / "raw"), str(tmp_path / "cache" / "dry_train")
    r = np.random.default_rng(0)
    _write_wav(os.path.join(src, "a.wav"), 48000, (0.1 * r.standard_normal(1600)).astype(np.float32))
    _write_wav(os.path.join(src, "sub", "deep", "b.wav"), 48000, (0.1 * r.standard_normal((800, 2))).astype(np.float32))
    _write_wav(os.path.join(src, "sub", "c.wav"), 44100, (3000 * r.standard_normal(500)).astype(np.int16))
    open(os.path.join(src, "notes.txt"), "w").write("not audio")
    launches = []

    def fake_rows(x, sr_in, sr_out, plan=None, out=None):         # the launch: rows of ceil(n up / down) samples
        launches.append((tuple(x.shape), sr_in, sr_out, plan.up, plan.down))
        n_out = -(-x.shape[1] * plan.up // plan.down)
        return x[:, :1].expand(x.shape[0], n_out) * 0.5

    monkeypatch.setattr(resample, "resample_rows", fake_rows)
    done = resample.convert_tree(src, dst, 44100, device="cpu")
    a, b, c = (os.path.join(src, p) for p in ("a.wav", "sub/deep/b.wav", "sub/c.wav"))
    assert done == {a: (48000, 1600, 1470), b: (48000, 800, 735), c: (44100, 500, 500)}
    assert launches == [((1, 1600), 48000, 44100, 147, 160), ((2, 800), 48000, 44100, 147, 160)]
    files = sorted(os.path.relpath(os.path.join(d, f), dst) for d, _, fs in os.walk(dst) for f in fs)
    assert files == sorted(p + s for p in ("a.wav", "sub/deep/b.wav", "sub/c.wav") for s in ("", resample.STAMP_SUFFIX))
    assert datasets.wav_info(os.path.join(dst, "a.wav")) == (1470, 44100, 1)
    assert datasets.wav_info(os.path.join(dst, "sub/deep/b.wav")) == (735, 44100, 2)
    got, _ = datasets.wav_load(os.path.join(dst, "sub/deep/b.wav"))
    assert got.dtype == torch.float32 and torch.equal(got, datasets.wav_load(b)[0][:, :1].expand(2, 735) * 0.5)
    assert open(os.path.join(dst, "sub/c.wav"), "rb").read() == open(c, "rb").read()          # at the rate already: the bytes
    stamp = json.load(open(os.path.join(dst, "a.wav" + resample.STAMP_SUFFIX)))
    st = os.stat(a)
    assert stamp == {"src_size": st.st_size, "src_mtime_ns": st.st_mtime_ns, "sr": 44100, "sr_in": 48000, "frames_in": 1600,
                     "frames_out": 1470, "filter": [48, 0.95, 16.0]}
    # a second run converts nothing and touches nothing
    before = {f: os.stat(os.path.join(dst, f)).st_mtime_ns for f in files}
    launches.clear()
    assert resample.convert_tree(src, dst, 44100, device="cpu") == done and launches == []
    assert {f: os.stat(os.path.join(dst, f)).st_mtime_ns for f in files} == before
    # a source that changed, a lost output and another filter are converted again; the others are not
    _write_wav(a, 48000, (0.1 * r.standard_normal(3200)).astype(np.float32))
    os.remove(os.path.join(dst, "sub/deep/b.wav"))
    assert resample.convert_tree(src, dst, 44100, device="cpu")[a] == (48000, 3200, 2940)
    assert [l[0] for l in launches] == [(1, 3200), (2, 800)]
    launches.clear()
    resample.convert_tree(src, dst, 44100, device="cpu", zeros=32, beta=12.0)
    assert len(launches) == 2 and json.load(open(os.path.join(dst, "a.wav" + resample.STAMP_SUFFIX)))["filter"] == [32, 0.95, 12.0]
    assert not [f for d, _, fs in os.walk(dst) for f in fs if ".tmp" in f]                     # no temporary name is left
    with pytest.raises(ValueError, match="differ"):
        resample.convert_tree(src, src, 44100, device="cpu")
    # the datasets read the converted tree, and say what they dropped from the raw one
    ds = datasets.RandomAudioChunkDataset(dst, 400, 44100, check_dataset=False)
    assert sorted(os.path.relpath(p, dst) for p in ds.input_paths) == ["a.wav", "sub/c.wav", "sub/deep/b.wav"]


def test_dropped_rates_are_named_once(tmp_path, caplog):
    from mod_extraction_amd import datasets
    src = str(tmp_path / "raw")
    z = np.zeros(1000, dtype=np.float32)
    for name, sr in (("a.wav", 48000), ("b.wav", 48000), ("c.wav", 96000), ("d.wav", 44100)):
        _write_wav(os.path.join(src, name), sr, np.zeros(1000 * sr // 44100, dtype=np.float32))
    _write_wav(os.path.join(src, "short.wav"), 48000, z[:100])                  # too short at any rate: not counted
    with caplog.at_level("WARNING", logger="mod_extraction_amd.datasets"):
        ds = datasets.RandomAudioChunkDataset(src, 500, 44100, check_dataset=False)
    assert [os.path.basename(p) for p in ds.input_paths] == ["d.wav"]
    warned = [r.getMessage() for r in caplog.records if r.name == "mod_extraction_amd.datasets"]
    assert len(warned) == 1 and "3 files" in warned[0] and "2 at 48000 Hz" in warned[0] and "1 at 96000 Hz" in warned[0]
    assert "resample_cache_dir" in warned[0] and "resample_dir.py" in warned[0]
    caplog.clear()
    with caplog.at_level("WARNING", logger="mod_extraction_amd.datasets"):
        datasets.RandomAudioChunkDataset(src, 500, 44100.0, check_dataset=False)
        os.remove(os.path.join(src, "a.wav")), os.remove(os.path.join(src, "b.wav")), os.remove(os.path.join(src, "c.wav"))
        n = len(caplog.records)
        datasets.RandomAudioChunkDataset(src, 500, 44100, check_dataset=False)
    assert n == 1 and len(caplog.records) == 1                                  # nothing dropped for its rate: no warning

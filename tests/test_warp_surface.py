"""CPU: the surface of the warp (K26) -- the declarations of mod_extraction_amd/csrc/warp_abi.h against ``_hip.SIGNATURES_WARP``
with the other four tables untouched, the argument checks and limits of the two entry points and of ``alignment.warp_rows`` /
``estimate_file_drift`` / ``warp_tree`` (all before any launch, in the documented order, so without a device), a stale
library, the defaults that keep ``score_pair`` and the data module the parent's, and the shipped config.  No device work."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from tests.helpers import warp64 as h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mod_extraction_amd", "csrc")
ABI_H = os.path.join(CSRC, "warp_abi.h")
ARG, UNSUPPORTED = -1, -2
NAMES = ["mx_warp_plan", "mx_warp_rows"]


def declared():
    """name -> parameter count of every ``int mx_*(...);`` of the header, read with this test's own regex."""
    text = re.sub(r"/\*.*?\*/", " ", open(ABI_H).read(), flags=re.S)
    return {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"^int\s+(mx_\w+)\s*\(([^;]*)\)\s*;", text, flags=re.M)}


def define(name):
    return re.search(rf"#define\s+{name}\s+(\S+)", open(ABI_H).read()).group(1)


def test_header_table_and_symbols():
    from mod_extraction_amd import _hip, alignment, build
    lib = ctypes.CDLL(build.build(verbose=False))
    counts = declared()
    assert list(counts) == list(_hip.SIGNATURES_WARP) == NAMES
    assert counts == {"mx_warp_plan": 11, "mx_warp_rows": 14}
    others = (_hip.SIGNATURES, _hip.SIGNATURES_TRACK, _hip.SIGNATURES_RESAMPLE, _hip.SIGNATURES_RATE)
    assert not any(n in t for n in counts for t in others)
    # the other four tables and the ABI number did not move
    assert len(_hip.SIGNATURES) == 124 and _hip.ABI_VERSION == 21 == lib.mx_abi_version()
    assert list(_hip.SIGNATURES_TRACK) == ["mx_track_fit_plan", "mx_track_fit"]
    assert list(_hip.SIGNATURES_RESAMPLE) == ["mx_resample_plan", "mx_resample_taps", "mx_resample_rows"]
    assert list(_hip.SIGNATURES_RATE) == ["mx_rate_track_plan", "mx_rate_track_nodes", "mx_rate_track_path", "mx_rate_track_refine"]
    text = open(os.path.join(ROOT, "include", "modex_hip.h")).read()
    assert "mx_warp" not in text and "MX_WARP" not in text and "warp_abi" not in text
    assert _hip.parse_signatures(text) == _hip.SIGNATURES
    bound = _hip.load()
    zeros = {ctypes.c_void_p: None, ctypes.c_int64: 0, ctypes.c_int32: 0, ctypes.c_float: 0.0, ctypes.c_double: 0.0}
    for name, n_args in counts.items():
        assert hasattr(lib, name) and len(_hip.SIGNATURES_WARP[name]) == n_args
        fn = getattr(bound, name)
        assert fn.argtypes == _hip.SIGNATURES_WARP[name] and fn.restype is ctypes.c_int       # load() binds the fifth table
        assert fn(*[zeros[t] for t in _hip.SIGNATURES_WARP[name]]) == ARG                     # all-zero arguments are refused
    src = open(os.path.join(CSRC, "warp.hip")).read()
    assert '#include "warp_abi.h"' in src and '#include "rows_common.h"' in src
    assert "warp_abi" not in open(os.path.join(CSRC, "common.h")).read()
    assert int(define("MX_WARP_OUT_TILE")) == h.OUT_TILE == _hip.WARP_OUT_TILE
    assert float(define("MX_WARP_MAX_DRIFT")) == h.MAX_DRIFT == _hip.WARP_MAX_DRIFT == alignment.MAX_DRIFT == 1e-3
    assert float(define("MX_WARP_MAX_OFFSET")) == alignment.MAX_OFFSET == 2.0 ** 31
    assert define("MX_WARP_MAX_TAPS") == "4095" and define("MX_WARP_MAX_ROWS") == "65535" and define("MX_WARP_MAX_N") == "(1LL"
    assert 0.95 * (1.0 + 1e-3) <= 1.0                                           # the default cut-off needs no scaling


def test_a_stale_library_names_the_fifth_header(monkeypatch):
    from mod_extraction_amd import _hip, build
    build.build(verbose=False)
    monkeypatch.setattr(_hip, "_lib", None)
    monkeypatch.setattr(_hip, "SIGNATURES_WARP", dict(_hip.SIGNATURES_WARP, mx_warp_of_tomorrow=[ctypes.c_void_p]))
    with pytest.raises(_hip.HipLibraryError, match=r"mx_warp_of_tomorrow.*csrc/warp_abi\.h.*rebuild.*python -m mod_extraction_amd\.build"):
        _hip.load()
    monkeypatch.undo()
    assert _hip.load() is not None


def lib_plan(zeros=48, rolloff=0.95, beta=16.0, n_in=1000, n_out=900, drift=0.0, offset=0.0, null=None):
    """(status, half, taps, tiles, span) of ``mx_warp_plan``; ``null``: the index of a missing output."""
    from mod_extraction_amd import _hip
    i32, i64 = (ctypes.c_int32 * 3)(-7, -7, -7), (ctypes.c_int64 * 1)(-7)
    a = ctypes.addressof(i32)
    outs = [a, a + 4, ctypes.addressof(i64), a + 8]
    if null is not None:
        outs[null] = None
    rc = _hip.load().mx_warp_plan(zeros, rolloff, beta, n_in, n_out, drift, offset, *outs)
    return rc, i32[0], i32[1], i64[0], i32[2]


def lib_rows(x=1 << 20, x_stride=None, B=2, n_in=1000, offset=1 << 30, drift=1 << 31, sign=None, zeros=48, rolloff=0.95, beta=16.0,
             y=1 << 40, y_stride=None, n_out=900):
    """``mx_warp_rows`` on pointers that are never read: every case below is refused before a launch."""
    from mod_extraction_amd import _hip
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    return _hip.load().mx_warp_rows(p(x), n_in if x_stride is None else x_stride, B, n_in, p(offset), p(drift), p(sign), zeros,
                                    rolloff, beta, p(y), n_out if y_stride is None else y_stride, n_out, None)


def test_plan_checks_and_limits():
    st = lambda **kw: lib_plan(**kw)[0]
    half, T = h.plan()
    assert lib_plan() == (0, half, T, 1, 1026 + T + 2) and (half, T) == (51, 103)
    assert lib_plan(n_out=1024)[3] == 1 and lib_plan(n_out=1025)[3] == 2
    for k in range(4):
        assert lib_plan(null=k) == (ARG, -7, -7, -7, -7)                        # a refused plan writes nothing
    assert st(zeros=0) == ARG and st(n_in=0) == ARG and st(n_out=0) == ARG
    assert st(rolloff=0.0) == ARG and st(rolloff=1.01) == ARG and st(rolloff=float("nan")) == ARG
    assert st(beta=-0.1) == ARG and st(beta=float("nan")) == ARG
    assert st(drift=-1e-9) == ARG and st(drift=float("nan")) == ARG and st(offset=-1.0) == ARG and st(offset=float("nan")) == ARG
    assert st(beta=64.0) == 0 and st(beta=64.5) == UNSUPPORTED
    assert st(zeros=2047, rolloff=1.0) == 0 and st(zeros=2048, rolloff=1.0) == UNSUPPORTED          # T = 4095, 4097
    assert st(n_in=1 << 40) == 0 and st(n_in=(1 << 40) + 1) == UNSUPPORTED and st(n_out=(1 << 40) + 1) == UNSUPPORTED
    assert st(drift=1e-3) == 0 and st(drift=1.0000001e-3) == UNSUPPORTED
    assert st(offset=2.0 ** 31 - 1) == 0 and st(offset=2.0 ** 31) == UNSUPPORTED
    # the order: arguments before limits; among the limits beta, T, n, then the two bounds
    assert st(zeros=0, beta=65.0) == ARG and st(drift=-1.0, beta=65.0) == ARG
    assert st(beta=65.0, drift=1.0) == UNSUPPORTED


def test_rows_checks_before_any_launch():
    assert lib_rows(x=None) == ARG and lib_rows(offset=None) == ARG and lib_rows(drift=None) == ARG and lib_rows(y=None) == ARG
    assert lib_rows(B=0) == ARG and lib_rows(n_in=0) == ARG and lib_rows(n_out=0) == ARG
    assert lib_rows(x_stride=999) == ARG and lib_rows(y_stride=899) == ARG
    assert lib_rows(zeros=0) == ARG and lib_rows(rolloff=0.0) == ARG and lib_rows(rolloff=1.5) == ARG and lib_rows(beta=-1.0) == ARG
    assert lib_rows(beta=65.0) == UNSUPPORTED and lib_rows(zeros=2048, rolloff=1.0) == UNSUPPORTED
    assert lib_rows(n_in=(1 << 40) + 1) == UNSUPPORTED and lib_rows(n_out=(1 << 40) + 1) == UNSUPPORTED
    # order: a short stride before a limit, a limit before an overlap
    assert lib_rows(x_stride=3, beta=65.0) == ARG and lib_rows(beta=65.0, y=1 << 20) == UNSUPPORTED
    # y shares a byte with x, with a parameter array or with the signs
    assert lib_rows(y=(1 << 20) + 4 * 1999) == ARG and lib_rows(y=(1 << 20) - 4 * 1799) == ARG
    assert lib_rows(y=(1 << 30) + 15) == ARG and lib_rows(y=(1 << 31) + 8) == ARG
    assert lib_rows(sign=1 << 41, y=(1 << 41) + 4) == ARG and lib_rows(sign=1 << 41, y=(1 << 41) - 4 * 1799) == ARG


def test_python_checks_in_their_order():
    """``warp_rows`` / ``warp_plan`` / ``estimate_file_drift`` / ``warp_tree`` on CPU tensors: every refusal comes before the
    device is asked for, and the LAST one is the device's."""
    from mod_extraction_amd import alignment as A
    x = torch.zeros(2, 100)
    with pytest.raises(ValueError, match="x must be an fp32"):
        A.warp_rows(x.double(), 0.0, 0.0)
    with pytest.raises(ValueError, match="x must be an fp32"):
        A.warp_rows(torch.zeros(1, 2, 3), 0.0, 0.0)
    with pytest.raises(ValueError, match="inner stride 1"):
        A.warp_rows(torch.zeros(100, 2).t(), 0.0, 0.0)
    with pytest.raises(ValueError, match="n_out must be an int >= 1"):
        A.warp_rows(x, 0.0, 0.0, n_out=0)
    with pytest.raises(ValueError, match="offset must be a float"):
        A.warp_rows(x, "1", 0.0)
    with pytest.raises(ValueError, match="drift must be a float"):
        A.warp_rows(x, 0.0, float("nan"))
    with pytest.raises(ValueError, match="zeros must be an int"):
        A.warp_rows(x, 0.0, 0.0, zeros=1.5)
    with pytest.raises(ValueError, match="need zeros"):
        A.warp_rows(x, 0.0, 0.0, rolloff=1.5)
    with pytest.raises(ValueError, match="beyond the warp's limits"):
        A.warp_rows(x, 0.0, 1.1e-3)
    with pytest.raises(ValueError, match="beyond the warp's limits"):
        A.warp_rows(x, 2.0 ** 31, 0.0)
    with pytest.raises(ValueError, match=r"offset must be a float or a \(2,\) fp64"):
        A.warp_rows(x, torch.zeros(2), 0.0)
    with pytest.raises(ValueError, match=r"drift must be a float or a \(2,\) fp64"):
        A.warp_rows(x, 0.0, torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="polarity must be"):
        A.warp_rows(x, 0.0, 0.0, polarity=2)
    with pytest.raises(ValueError, match="polarity must be"):
        A.warp_rows(x, 0.0, 0.0, polarity=torch.zeros(2, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"out must be an fp32 tensor of shape \(2, 50\)"):
        A.warp_rows(x, 0.0, 0.0, n_out=50, out=torch.zeros(2, 51))
    with pytest.raises(ValueError, match="rows of out overlap"):
        A.warp_rows(x, 0.0, 0.0, n_out=50, out=torch.zeros(50).expand(2, 50))
    with pytest.raises(ValueError, match="out may not overlap"):
        A.warp_rows(x, 0.0, 0.0, out=x)
    off = torch.zeros(50, dtype=torch.float64)
    with pytest.raises(ValueError, match="out may not overlap"):
        A.warp_rows(x, off[:2], 0.0, n_out=50, out=off.view(torch.float32).view(2, 50))
    with pytest.raises(ValueError, match="HIP device"):                         # everything else is in order: the device is last
        A.warp_rows(x, 0.5, 1e-4, n_out=70, polarity=-1, out=torch.zeros(2, 70))
    assert A.warp_plan(1000, 900) == (51, 103, 1, 1131) and A.warp_plan(5, 4097, zeros=4, rolloff=1.0)[:3] == (4, 9, 5)
    with pytest.raises(ValueError, match="limits"):
        A.warp_plan(10, 10, max_drift=2e-3)

    d, w = torch.zeros(20000), torch.zeros(20040)
    est = lambda *a, **kw: A.estimate_file_drift(*a, **kw)
    with pytest.raises(ValueError, match="max_lag must be an int"):
        est(d, w, 1.5)
    with pytest.raises(ValueError, match="probe_points must be an int >= 2"):
        est(d, w, 10, probe_points=1)
    with pytest.raises(ValueError, match="n_probes must be an int >= 2"):
        est(d, w, 10, n_probes=1)
    with pytest.raises(ValueError, match=r"max_lag must be in 0 \.\. min\(8192, probe_points - 1\) = 63"):
        est(d, w, 64, probe_points=64)
    with pytest.raises(ValueError, match=r"= 8192, got 8193"):
        est(d, w, 8193, probe_points=16384)
    with pytest.raises(ValueError, match="min_probes"):
        est(d, w, 10, min_probes=1)
    with pytest.raises(ValueError, match="min_corr"):
        est(d, w, 10, min_corr=1.5)
    with pytest.raises(ValueError, match="dry must be an fp32 tensor of shape"):
        est(d.view(1, -1), w, 10)
    with pytest.raises(ValueError, match="wet must be an fp32 tensor of shape"):
        est(d, w.double(), 10)
    with pytest.raises(ValueError, match="shorter than one probe"):
        est(d, w[:8000], 10)
    with pytest.raises(ValueError, match="one HIP device"):
        est(d, w, 10)
    assert A.probe_starts(20000, 20040, 8192, 16) == ((20000 - 8192) // 15, 20000 - 8192)


def test_warp_tree_checks(tmp_path):
    from mod_extraction_amd import alignment as A
    a, b, c = (str(tmp_path / n) for n in "abc")
    with pytest.raises(ValueError, match="sr must be an int"):
        A.warp_tree(a, b, c, 44100.0, 100)
    with pytest.raises(ValueError, match="max_lag must be in"):
        A.warp_tree(a, b, c, 44100, 9000)
    with pytest.raises(ValueError, match="min_drift_samples"):
        A.warp_tree(a, b, c, 44100, 100, min_drift_samples=-1.0)
    with pytest.raises(ValueError, match="limits"):
        A.warp_tree(a, b, c, 44100, 100, beta=70.0)
    with pytest.raises(ValueError, match="three directories"):
        A.warp_tree(a, b, b, 44100, 100)


def test_defaults_leave_the_parent_alone(tmp_path):
    from mod_extraction_amd import alignment, data_modules, datasets, file_eval
    assert inspect.signature(file_eval.score_pair).parameters["drift"].default is None
    assert list(inspect.signature(file_eval.score_pair).parameters)[-1] == "drift"           # appended: positional calls keep their meaning
    # the data module without the key builds the parent's datasets on the directories it was given, and warps nothing
    import numpy as np
    r = np.random.default_rng(0)
    for d in ("dry", "wet"):
        os.makedirs(tmp_path / d)
        datasets.wav_save(str(tmp_path / d / "a.wav"), torch.from_numpy(r.standard_normal((1, 4000)).astype(np.float32) * 0.1), 8000)
    called = []
    orig = alignment.warp_tree
    alignment.warp_tree = lambda *a, **kw: called.append(a) or orig(*a, **kw)
    try:
        dm = data_modules.RandomAudioChunkDryWetDataModule(batch_size=2, n_samples=1000, sr=8000, dry_train_dir=str(tmp_path / "dry"),
                                                           wet_train_dir=str(tmp_path / "wet"), check_dataset=False)
        dm.setup(torch.device("cpu"))
        ds = dm._pairs["train"]
        assert ds.wet_dir == str(tmp_path / "wet") and ds.dry_dir == str(tmp_path / "dry") and not called
        assert dm.pair_drift == {"train": None, "val": None} and dm.pair_alignment == {"train": None, "val": None}
        needs = data_modules.RandomAudioChunkDryWetDataModule(batch_size=2, n_samples=1000, sr=8000, dry_train_dir=str(tmp_path / "dry"),
                                                              wet_train_dir=str(tmp_path / "wet"), check_dataset=False,
                                                              align_drift_cache_dir=str(tmp_path / "cache"))
        with pytest.raises(ValueError, match="align_drift_cache_dir needs align_max_lag_ms"):
            needs.setup(torch.device("cpu"))
    finally:
        alignment.warp_tree = orig
    assert sorted(os.listdir(tmp_path)) == ["dry", "wet"]


def test_shipped_config():
    """train_lfo_pairs_flanger_drift.yml is train_lfo_pairs_flanger_fir.yml plus the three keys, and K21's inequality holds:
    the FIR's window stays below the flanger's smallest delay."""
    import yaml
    from mod_extraction_amd import cli, lightning
    load = lambda name: yaml.safe_load(open(os.path.join(ROOT, "configs", name)))
    new, base = load("train_lfo_pairs_flanger_drift.yml"), load("train_lfo_pairs_flanger_fir.yml")
    data = new["data"]["init_args"]
    assert data.pop("align_drift_cache_dir") == "../data/flanger_pairs/undrifted" and data.pop("align_drift_n_probes") == 16
    assert round(data.pop("align_drift_probe_ms") * 1e-3 * data["sr"]) == 8192
    assert new == base
    # the reach: align_max_lag_ms is within a probe and within K19's limit; 8192 points at 100 ppm move 0.8 samples
    assert round(data["align_max_lag_ms"] * 1e-3 * data["sr"]) <= min(8192, 8192 - 1)
    old = os.getcwd()
    os.chdir(os.path.join(ROOT, "scripts"))
    try:
        c = cli.CustomLightningCLI(args=["fit", "-c", "../configs/train_lfo_pairs_flanger_drift.yml"], run=False, device=torch.device("cpu"))
    finally:
        os.chdir(old)
    assert isinstance(c.model, lightning.LFOExtractionThroughEffect) and c.model.match_fir == 9
    fixed = new["model"]["init_args"]["learned_fx"]["flanger"]["min_delay_width"]
    assert isinstance(fixed, float)
    assert c.model.match_fir - 1 - c.model.match_fir_centre < fixed * c.model.max_min_delay_samples

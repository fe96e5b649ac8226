"""CPU: the surface of the pair alignment (K19) -- its declarations in include/modex_hip.h against ``_hip.SIGNATURES``,
the limits of the three entry points (checked before any launch, so without a device), the ``ValueError``s of the wrappers
in ``mod_extraction_amd.alignment``, ``PairLag``, and the shipped config.  No device work."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"mx_pair_xcorr": 9, "mx_pair_peak": 12, "mx_pair_shift": 9}
ARG, UNSUPPORTED = -1, -2


def test_header_table_and_symbols():
    """Three entry points, declared in include/modex_hip.h (section K19) and bound from ``_hip.SIGNATURES``, which is derived
    from that text."""
    from mod_extraction_amd import _hip, build
    from tests.test_abi import header_arg_counts
    lib = ctypes.CDLL(build.build(verbose=False))
    assert {k: v for k, v in header_arg_counts().items() if k.startswith("mx_pair_")} == NAMES
    assert {k: len(v) for k, v in _hip.SIGNATURES.items() if k.startswith("mx_pair_")} == NAMES
    assert _hip.ABI_VERSION == 21 == lib.mx_abi_version()
    zeros = {ctypes.c_void_p: None, ctypes.c_int64: 0, ctypes.c_int32: 0, ctypes.c_float: 0.0}
    for name in NAMES:
        assert hasattr(lib, name)
        fn = getattr(_hip.load(), name)
        assert fn.argtypes == _hip.SIGNATURES[name]                           # load() binds the table
        assert fn(*[zeros[t] for t in fn.argtypes]) == ARG


def p(v):
    return None if v is None else ctypes.c_void_p(v)


def xcorr(dry=8, wet=8, B=4, N=1000, L=10, ds=None, ws=None, r=8):
    from mod_extraction_amd import _hip
    return _hip.load().mx_pair_xcorr(p(dry), N if ds is None else ds, p(wet), N if ws is None else ws, B, N, L, p(r), None)


def peak(dry=8, wet=8, r=8, B=4, N=1000, L=10, ds=None, ws=None, out=(8, 8, 8)):
    from mod_extraction_amd import _hip
    return _hip.load().mx_pair_peak(p(dry), N if ds is None else ds, p(wet), N if ws is None else ws, p(r), B, N, L,
                                    *[p(o) for o in out], None)


def shift(wet=8, B=4, N=1000, lag=8, corr=None, out=1 << 30, ws=None, os_=None):
    from mod_extraction_amd import _hip
    return _hip.load().mx_pair_shift(p(wet), N if ws is None else ws, B, N, p(lag), p(corr), p(out), N if os_ is None else os_,
                                     None)


def test_limits_are_checked_before_any_launch():
    """Every case is refused on pointers that are never read (a case that would launch is not tried here)."""
    for fn in (xcorr, peak):
        assert fn(dry=None) == ARG and fn(wet=None) == ARG and fn(r=None) == ARG
        assert fn(B=0) == ARG and fn(B=-2) == ARG and fn(N=0) == ARG and fn(N=-5, L=0) == ARG
        assert fn(L=-1) == ARG and fn(L=1000) == ARG and fn(N=5, L=5) == ARG and fn(L=5000) == ARG
        assert fn(ds=999) == ARG and fn(ws=999) == ARG
        assert fn(N=(1 << 24) + 1) == UNSUPPORTED and fn(N=20000, L=8193) == UNSUPPORTED and fn(B=65536) == UNSUPPORTED
    for k in range(3):
        assert peak(out=[None if i == k else 8 for i in range(3)]) == ARG, k
    assert shift(wet=None) == ARG and shift(lag=None) == ARG and shift(out=None) == ARG
    assert shift(B=0) == ARG and shift(N=0) == ARG and shift(ws=999) == ARG and shift(os_=999) == ARG
    assert shift(N=(1 << 24) + 1) == UNSUPPORTED and shift(B=65536) == UNSUPPORTED
    # out may not overlap wet: 4 rows of 1000 floats from address 4096 end at 4096 + 16000
    assert shift(wet=4096, out=4096) == ARG and shift(wet=4096, out=4096 + 15996) == ARG and shift(wet=4096 + 15996, out=4096) == ARG


class Fake:
    """Stands in for a device tensor where only the checks before the launch are under test."""


def test_wrapper_errors_are_raised_before_the_launch(monkeypatch):
    from mod_extraction_amd import _hip, alignment as A
    calls = []
    monkeypatch.setattr(_hip, "call", lambda name, *a: calls.append(name))
    d, w = torch.zeros(3, 48), torch.zeros(3, 48)
    for fn in (A.xcorr_lags, A.estimate_pair_lag, A.align_pairs):
        with pytest.raises(ValueError, match="no CPU fallback"):
            fn(d, w, 4)                                                       # CPU tensors
        with pytest.raises(ValueError, match="fp32"):
            fn(d.double(), w, 4)
        with pytest.raises(ValueError, match="fp32"):
            fn(d.to(torch.int32), w, 4)
        with pytest.raises(ValueError, match="fp32"):
            fn(torch.zeros(3, 2, 48), w, 4)                                   # (B, C, N) with C != 1
        with pytest.raises(ValueError, match="fp32"):
            fn(torch.zeros(1, 1, 3, 48), w, 4)
        with pytest.raises(ValueError, match="fp32"):
            fn([0.0] * 48, w, 4)
    with pytest.raises(ValueError, match="no CPU fallback"):
        A.shift_rows(w, torch.zeros(3, dtype=torch.int32))
    assert calls == []
    assert A.MAX_LAG == 8192


def test_wrapper_shape_and_lag_errors(monkeypatch):
    """The checks behind the device check, on meta tensors that say they are on a HIP device."""
    from mod_extraction_amd import _hip, alignment as A
    calls = []
    monkeypatch.setattr(_hip, "call", lambda name, *a: calls.append(name))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    d, w = torch.zeros(3, 48), torch.zeros(3, 48)
    for fn in (A.xcorr_lags, A.estimate_pair_lag, A.align_pairs):
        with pytest.raises(ValueError, match="same rows"):
            fn(d, torch.zeros(3, 47), 4)
        with pytest.raises(ValueError, match="same rows"):
            fn(d, torch.zeros(2, 48), 4)
        with pytest.raises(ValueError, match="wet must be an fp32"):
            fn(d, w.to(torch.int32), 4)
        for bad in (-1, 48, 8193, 2.0, None, True):
            with pytest.raises(ValueError, match="max_lag"):
                fn(d, w, bad)
        with pytest.raises(ValueError, match="no rows"):
            fn(torch.zeros(0, 48), torch.zeros(0, 48), 4)
    with pytest.raises(ValueError, match="max_lag"):
        A.xcorr_lags(torch.zeros(2, 9000), torch.zeros(2, 9000), 8193)        # min(8192, N - 1)
    lag = torch.zeros(3, dtype=torch.int32)
    for bad in (lag.long(), torch.zeros(2, dtype=torch.int32), [0, 0, 0]):
        with pytest.raises(ValueError, match="lag must be"):
            A.shift_rows(w, bad)
    for bad in (torch.zeros(3, dtype=torch.float64), torch.zeros(4), 1.0):
        with pytest.raises(ValueError, match="corr must be"):
            A.shift_rows(w, lag, bad)
    for bad in (torch.zeros(3, 47), torch.zeros(3, 48, dtype=torch.float64), torch.zeros(3, 1, 48)):
        with pytest.raises(ValueError, match="out must be"):
            A.shift_rows(w, lag, out=bad)
    with pytest.raises(ValueError, match="inner stride"):
        A.shift_rows(w, lag, out=torch.zeros(3, 96)[:, ::2])
    with pytest.raises(ValueError, match="overlap"):
        A.shift_rows(w, lag, out=w)
    big = torch.zeros(3, 100)
    with pytest.raises(ValueError, match="overlap"):
        A.shift_rows(big[:, :48], lag, out=big[:, 50:98])                     # interleaved rows of one buffer
    assert calls == []


def test_pairlag_is_a_named_tuple():
    from mod_extraction_amd import alignment as A
    v = [torch.zeros(3, dtype=torch.int32), torch.zeros(3), torch.ones(3)]
    e = A.PairLag(*v)
    assert e._fields == ("lag", "frac", "corr") and e.lag is v[0] and e.frac is v[1] and e.corr is v[2]


def test_shipped_config():
    """train_lfo_pairs_flanger_aligned.yml is train_lfo_pairs_flanger.yml plus the alignment keys and an end buffer that
    covers the largest lag."""
    from mod_extraction_amd import cli, data_modules
    old = os.getcwd()
    os.chdir(os.path.join(ROOT, "scripts"))
    try:
        mk = lambda name: cli.CustomLightningCLI(args=["fit", "-c", f"../configs/{name}"], run=False,
                                                 device=torch.device("cpu"))
        c, base = mk("train_lfo_pairs_flanger_aligned.yml"), mk("train_lfo_pairs_flanger.yml")
    finally:
        os.chdir(old)
    assert isinstance(c.datamodule, data_modules.RandomAudioChunkDryWetDataModule)
    extra = {"align_max_lag_ms": 50.0, "align_n_probes": 8, "align_min_corr": 0.5, "end_buffer_n_samples": 2205}
    init = c.config["data"]["init_args"]
    assert {k: init[k] for k in extra} == extra
    assert init["end_buffer_n_samples"] >= round(init["align_max_lag_ms"] * 1e-3 * init["sr"])
    assert {k: v for k, v in init.items() if k not in extra} == base.config["data"]["init_args"]
    assert c.config["model"] == base.config["model"]
    for k in extra:
        assert c.datamodule.ignored_args[k] == extra[k] and k not in base.datamodule.ignored_args
    assert c.datamodule.pair_alignment == {"train": None, "val": None}

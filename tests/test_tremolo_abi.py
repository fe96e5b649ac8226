"""CPU: the tremolo entry points are part of the C ABI -- declared in the binding table, exported by the library, behind
ABI version 21, and they refuse null pointers before touching the device."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def so_path():
    from mod_extraction_amd import build
    return build.build(verbose=False)


def test_tremolo_entry_points_are_bound_and_exported(so_path):
    from mod_extraction_amd import _hip
    lib = ctypes.CDLL(so_path)
    for name in ("mx_tremolo_fwd", "mx_tremolo_bwd"):
        assert name in _hip.SIGNATURES, name
        assert hasattr(lib, name), name
    assert len(_hip.SIGNATURES["mx_tremolo_fwd"]) == 13 and len(_hip.SIGNATURES["mx_tremolo_bwd"]) == 17


def test_abi_version_is_21(so_path):
    from mod_extraction_amd import _hip
    assert _hip.ABI_VERSION == 21
    assert _hip.load().mx_abi_version() == 21


def test_null_pointers_are_refused(so_path):
    from mod_extraction_amd import _hip
    lib = _hip.load()
    zeros = {ctypes.c_void_p: None, ctypes.c_int64: 0}
    for name in ("mx_tremolo_fwd", "mx_tremolo_bwd"):
        assert getattr(lib, name)(*[zeros[t] for t in _hip.SIGNATURES[name]]) in (-1, -2), name
    # null pointers behind plausible sizes: still refused on the host
    fwd = [None, 64, None, 8, None, None, None, 0, 2, 64, None, 64, None]
    assert lib.mx_tremolo_fwd(*fwd) in (-1, -2)
    bwd = [None, 64, None, 64, None, 8, None, None, None, 0, 2, 64, None, 64, None, None, None]
    assert lib.mx_tremolo_bwd(*bwd) in (-1, -2)

"""CPU: the two low-rate phaser entry points are part of the C ABI -- in the binding table, exported by the library,
declared in the public header -- they refuse bad arguments on the host before any launch, and adding them did not move the
ABI version (21: new entry points are backward compatible)."""
import ctypes
import os

import pytest

NAMES = ("mx_phaser_mod_expand", "mx_phaser_dmod_gather")


@pytest.fixture(scope="module")
def so_path():
    from mod_extraction_amd import build
    return build.build(verbose=False)


def test_entry_points_are_bound_and_exported(so_path):
    from mod_extraction_amd import _hip
    lib = ctypes.CDLL(so_path)
    for name in NAMES:
        assert name in _hip.SIGNATURES, name
        assert hasattr(lib, name), name
        assert len(_hip.SIGNATURES[name]) == 9, name


def test_header_declares_them():
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "modex_hip.h")) as f:
        text = f.read()
    for name in NAMES:
        assert f"int {name}(" in text, name
    assert "K3c" in text and "no counterpart" in text[text.index("K3c"):text.index("mx_phaser_mod_expand(")]


def test_abi_version_is_still_21(so_path):
    from mod_extraction_amd import _hip
    assert _hip.ABI_VERSION == 21
    assert _hip.load().mx_abi_version() == 21


def test_bad_arguments_are_refused_on_the_host(so_path):
    from mod_extraction_amd import _hip
    lib = _hip.load()
    zeros = {ctypes.c_void_p: None, ctypes.c_int64: 0}
    for name in NAMES:
        assert getattr(lib, name)(*[zeros[t] for t in _hip.SIGNATURES[name]]) in (-1, -2), name
    # null pointers behind plausible sizes: (mod_lr, n_mod, lead, B, N, x_width, mod_g, mod_g_stride, stream)
    assert lib.mx_phaser_mod_expand(None, 8, None, 2, 64, 64, None, 16, None) in (-1, -2)
    # (dmod_g, dmod_g_stride, n_groups, lead, B, N, n_mod, dmod_lr, stream)
    assert lib.mx_phaser_dmod_gather(None, 16, 16, None, 2, 64, 8, None, None) in (-1, -2)
    # sizes that are wrong behind non-null pointers (never dereferenced on the host; no launch happens)
    buf = (ctypes.c_float * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for n_mod, N, width, stride in ((0, 64, 64, 16),       # n_mod < 1
                                    (65, 64, 64, 16),      # n_mod > N
                                    (8, 64, 63, 16),       # x_width < N
                                    (8, 64, 64, 15)):      # a stride shorter than the row
        assert lib.mx_phaser_mod_expand(p, n_mod, None, 2, N, width, p, stride, None) == -1, (n_mod, N, width, stride)
    for stride, groups, N, n_mod in ((15, 16, 64, 8),      # a stride shorter than the row
                                     (16, 15, 64, 8),      # fewer groups than the clip window has
                                     (16, 16, 64, 0),      # n_mod < 1
                                     (16, 16, 64, 65)):    # n_mod > N
        assert lib.mx_phaser_dmod_gather(p, stride, groups, None, 2, N, n_mod, p, None) == -1, (stride, groups, N, n_mod)

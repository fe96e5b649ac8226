"""CPU: the two row-listed low-rate phaser entry points (mx_phaser_mod_expand_rows / mx_phaser_dmod_gather_rows) are part of
the C ABI -- bound, exported, declared -- with 11 arguments each and the ABI version still 21; they refuse bad arguments on
the host before any launch (a NULL row list, n_rows < 1, n_rows > B: MX_ERR_ARG); and the fp64 reference of their contract
(tests/helpers/phaser_lr64_rows.py) keeps the transpose identity on the listed rows and leaves the others alone."""
import ctypes
import os

import numpy as np
import pytest

from tests.helpers.phaser_lr64 import expand64, gather64
from tests.helpers.phaser_lr64_rows import expand64_rows, gather64_rows

NAMES = ("mx_phaser_mod_expand_rows", "mx_phaser_dmod_gather_rows")


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
        assert len(_hip.SIGNATURES[name]) == 11, name
    assert _hip.ABI_VERSION == 21 and _hip.load().mx_abi_version() == 21


def test_header_declares_them():
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "modex_hip.h")) as f:
        text = f.read()
    for name in NAMES:
        assert f"int {name}(" in text, name
        decl = text[text.index(f"int {name}("):]
        assert decl[:decl.index(";")].count(",") == 10, name                         # 11 arguments
    comment = text[text.index("int mx_phaser_dmod_gather("):text.index("int mx_phaser_mod_expand_rows(")]
    assert "no counterpart" in comment and "NOT checked by the host" in comment and "neither read nor written" in comment


def test_bad_arguments_are_refused_on_the_host(so_path):
    from mod_extraction_amd import _hip
    lib = _hip.load()
    zeros = {ctypes.c_void_p: None, ctypes.c_int64: 0}
    for name in NAMES:
        assert getattr(lib, name)(*[zeros[t] for t in _hip.SIGNATURES[name]]) in (-1, -2), name
    buf = (ctypes.c_float * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)                 # never dereferenced on the host; no launch happens
    # (mod_lr, n_mod, lead, rows, n_rows, B, N, x_width, mod_g, mod_g_stride, stream)
    for rows, n_rows in ((None, 1), (p, 0), (p, -1), (p, 3)):                        # B = 2
        assert lib.mx_phaser_mod_expand_rows(p, 8, None, rows, n_rows, 2, 64, 64, p, 16, None) == -1, (rows, n_rows)
    for n_mod, N, width, stride in ((0, 64, 64, 16), (65, 64, 64, 16), (8, 64, 63, 16), (8, 64, 64, 15)):
        assert lib.mx_phaser_mod_expand_rows(p, n_mod, None, p, 1, 2, N, width, p, stride, None) == -1
    assert lib.mx_phaser_mod_expand_rows(None, 8, None, p, 1, 2, 64, 64, p, 16, None) == -1
    assert lib.mx_phaser_mod_expand_rows(p, 8, None, p, 1, 2, 64, 1 << 30, p, 1 << 28, None) == -2      # the grid limits
    # (dmod_g, dmod_g_stride, n_groups, lead, rows, n_rows, B, N, n_mod, dmod_lr, stream)
    for rows, n_rows in ((None, 1), (p, 0), (p, -1), (p, 3)):
        assert lib.mx_phaser_dmod_gather_rows(p, 16, 16, None, rows, n_rows, 2, 64, 8, p, None) == -1, (rows, n_rows)
    for stride, groups, N, n_mod in ((15, 16, 64, 8), (16, 15, 64, 8), (16, 16, 64, 0), (16, 16, 64, 65)):
        assert lib.mx_phaser_dmod_gather_rows(p, stride, groups, None, p, 1, 2, N, n_mod, p, None) == -1
    assert lib.mx_phaser_dmod_gather_rows(p, 16, 16, None, p, 1, 2, 64, 8, None, None) == -1
    assert lib.mx_phaser_dmod_gather_rows(p, 1 << 28, 1 << 28, None, p, 1, 2, 64, 8, p, None) == -2


@pytest.mark.parametrize("N,n_mod,rows", [(37, 5, [0, 3, 4]), (64, 64, [4, 1]), (5, 2, [0, 1, 2, 3, 4]), (222, 9, [2])])
def test_fp64_rows_reference_keeps_the_transpose_identity(N, n_mod, rows):
    rng = np.random.default_rng(N + n_mod)
    B, W = 5, N + 11
    lead = rng.integers(0, 12, B)
    ng = (W + 3) // 4
    m, d = rng.standard_normal((B, n_mod)), rng.standard_normal((B, ng))
    e = expand64_rows(m, lead, rows, N, W, np.full((B, ng), 7.0))
    g = gather64_rows(d, lead, rows, N, n_mod, np.full((B, n_mod), 7.0))
    other = [b for b in range(B) if b not in rows]
    assert np.all(e[other] == 7.0) and np.all(g[other] == 7.0)                    # rows that are not listed: untouched
    assert np.array_equal(e[rows], expand64(m, lead, N, W)[rows]) and np.array_equal(g[rows], gather64(d, lead, N, n_mod)[rows])
    # <expand(m) - expand(0), d> = <m, gather(d)> on the listed rows (the expand is affine: 0.5 beyond the clip)
    lin = e[rows] - expand64_rows(np.zeros_like(m), lead, rows, N, W, np.zeros((B, ng)))[rows]
    lhs, rhs = float((lin * d[rows]).sum()), float((m[rows] * g[rows]).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), (lhs, rhs)

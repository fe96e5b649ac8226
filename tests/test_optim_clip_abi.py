"""CPU: the two gradient-clipping entry points (mx_grad_sumsq / mx_adamw_step_clip, csrc/optim_clip.hip) are part of the C ABI
-- declared in the header, bound in the ctypes table with matching argument counts, exported by the library, behind the same
ABI version (21: new entry points are backward compatible) -- and refuse bad arguments before touching a device; the
workspace size `optim.sumsq_partials` restates what the header documents."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mx_grad_sumsq": 5, "mx_adamw_step_clip": 16}
MX_ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from mod_extraction_amd import _hip, build
    build.build(verbose=False)
    return _hip.load()


def _header():
    return open(os.path.join(ROOT, "include", "modex_hip.h")).read()


def test_entry_points_declared_bound_and_exported(lib):
    from mod_extraction_amd import _hip
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name, n_args in NEW.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, code, flags=re.S)
        assert m, f"{name} is not declared in include/modex_hip.h"
        assert len(m.group(1).split(",")) == n_args
        assert len(_hip.SIGNATURES[name]) == n_args
        assert hasattr(lib, name)
    assert _hip.ABI_VERSION == 21 and lib.mx_abi_version() == 21


def _sumsq_args(grad=1, n=8, part=1, stat=1):
    return [ctypes.c_void_p(grad or None), n, ctypes.c_void_p(part or None), ctypes.c_void_p(stat or None), None]


def _clip_args(param=1, grad=1, m=1, v=1, n=8, step=1, mode=1, clip=1.0, stat=1):
    P = lambda x: ctypes.c_void_p(x or None)                    # noqa: E731
    return [P(param), P(grad), P(m), P(v), n, step, 1e-4, 0.8, 0.99, 1e-8, 0.01, 1.0, mode, clip, P(stat), None]


@pytest.mark.parametrize("kw", [dict(grad=0), dict(part=0), dict(stat=0), dict(n=0), dict(n=-5)])
def test_sumsq_refuses_bad_arguments_without_a_device(lib, kw):
    assert lib.mx_grad_sumsq(*_sumsq_args(**kw)) == MX_ERR_ARG


@pytest.mark.parametrize("kw", [dict(param=0), dict(grad=0), dict(m=0), dict(v=0), dict(stat=0), dict(n=0), dict(step=0),
                                dict(mode=0), dict(mode=3), dict(mode=-1), dict(clip=0.0), dict(clip=-1.0),
                                dict(clip=float("inf")), dict(clip=float("nan"))])
def test_step_clip_refuses_bad_arguments_without_a_device(lib, kw):
    assert lib.mx_adamw_step_clip(*_clip_args(**kw)) == MX_ERR_ARG


def test_sumsq_partials_restates_the_header():
    from mod_extraction_amd import optim
    m = re.search(r"mx_sumsq_partials\(n\) = min\(ceil\(n / (\d+)\), (\d+)\)", _header())
    assert m, "include/modex_hip.h must document G(n)"
    chunk, cap = int(m.group(1)), int(m.group(2))
    assert (optim.SUMSQ_CHUNK, optim.SUMSQ_MAX_PARTIALS) == (chunk, cap)
    G = optim.sumsq_partials
    assert G(1) == 1 and G(chunk - 1) == 1 and G(chunk) == 1 and G(chunk + 1) == 2
    for g in (2, 3, 17, cap - 1):                                # both sides of every chunk boundary looked at
        assert G(g * chunk) == g and G(g * chunk + 1) == g + 1
    assert G(cap * chunk) == cap and G(cap * chunk + 1) == cap and G(1 << 40) == cap
    prev = 0
    for n in list(range(1, 3 * chunk + 2, 97)) + [cap * chunk - 1, cap * chunk, cap * chunk + 5, 10 ** 9]:
        assert G(n) >= max(1, prev)                              # monotone, never below 1
        prev = G(n)
    src = open(os.path.join(ROOT, "mod_extraction_amd", "csrc", "optim_clip.hip")).read()
    assert f"#define MX_SUMSQ_CHUNK {chunk}" in src and f"#define MX_SUMSQ_MAX_PARTIALS {cap}" in src

"""CPU: the C-ABI library loads and exports every symbol include/modex_hip.h declares, and the ctypes binding table, which
``_hip`` derives from that header, matches it (no compute calls -- there is no GPU here).  ``header_symbols`` and
``header_arg_counts`` read the header with a regex of their own, not with ``_hip.parse_signatures``, so that a mistake of
the parser cannot hide behind itself."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ENTRY_POINTS = 124                      # the one pin of the number of declarations; a new entry point raises it here


def header_symbols():
    text = open(os.path.join(ROOT, "include", "modex_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.findall(r"\bint\s+(mx_\w+)\s*\(", text)


def header_arg_counts():
    text = open(os.path.join(ROOT, "include", "modex_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(mx_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else len(args.split(","))
    return out


@pytest.fixture(scope="module")
def so_path():
    from mod_extraction_amd import build
    return build.build(verbose=False)


def test_library_exports_every_declared_symbol(so_path):
    lib = ctypes.CDLL(so_path)
    syms = header_symbols()
    assert len(syms) == len(set(syms)) == N_ENTRY_POINTS
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/modex_hip.h but not exported"
    assert lib.mx_abi_version() >= 1


def test_binding_table_matches_header(so_path):
    from mod_extraction_amd import _hip
    counts = header_arg_counts()
    assert len(counts) == N_ENTRY_POINTS and isinstance(_hip.SIGNATURES, dict)
    assert set(counts) == set(_hip.SIGNATURES), set(counts) ^ set(_hip.SIGNATURES)
    for name, n in counts.items():
        assert len(_hip.SIGNATURES[name]) == n, name
    lib = _hip.load()
    assert lib.mx_abi_version() == _hip.ABI_VERSION
    for name, argtypes in _hip.SIGNATURES.items():                            # load() binds the one table
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is ctypes.c_int, name


def test_parser_reads_every_parameter_kind():
    """The argtype lists of entries that between them use all seven kinds (pointer, int64, int32, uint64, uint32, float,
    double), written out by hand from the declarations: a parser that misreads a type fails here."""
    from mod_extraction_amd import _hip
    P, I64, I32, F32, F64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_double
    U64, U32 = ctypes.c_uint64, ctypes.c_uint32
    expected = {
        "mx_abi_version": [],
        "mx_uniform_rows": [P, I64, P, I64, P, I64, I64, U64, U32, F32, F32, P],
        "mx_lfo_synth": [P, P, P, P, P, I64, I64, I64, F32, P, P],
        "mx_phaser_fwd": [P, I64, P, P, P, P, P, P, P, I64, I64, I64, F64, I32, P, I64, P, P, I64, P],
        "mx_gain_match_apply": [P, I64, P, I64, I64, I32, F64, I32, F64, F64, P, I64, P, P, P, P],
        "mx_lfo_fit": [P, I64, I64, I64, F32, F32, F32, I32, I32, I32, I32, P, P, P, P, P, P, P, P],
        "mx_lstm_step_probe": [I32, I64, P, P],
    }
    for name, argtypes in expected.items():
        assert _hip.SIGNATURES[name] == argtypes, name
    assert {t for a in expected.values() for t in a} == {P, I64, I32, U64, U32, F32, F64}
    assert {t for a in _hip.SIGNATURES.values() for t in a} == {P, I64, I32, U64, U32, F32, F64}
    for name in _hip.PROBE_TWINS:                                             # the header declares the twins themselves
        assert _hip.SIGNATURES[name + "_probe"] == _hip.SIGNATURES[name] != [], name
    assert _hip.SIGNATURES == _hip.parse_signatures(open(os.path.join(ROOT, "include", "modex_hip.h")).read())
    # spellings the header may use: no parameter name, const on a scalar, a pointer to const, // comments, no space at the *
    text = "int mx_a(int64_t, const double x, const float *const p, uint32_t* q); // int mx_c(int n);\nint  mx_b ( void ) ;"
    assert _hip.parse_signatures(text) == {"mx_a": [I64, F64, P, P], "mx_b": []}


@pytest.mark.parametrize("text, named", [
    ("int mx_a(float *x, size_t n, void *stream);", ("mx_a", "size_t n")),
    ("int mx_a(float *x, int n, void *stream);", ("mx_a", "int n")),
    ("int mx_ok(void);\nint mx_a(struct mx_dims d, void *stream);", ("mx_a", "struct mx_dims d")),
    ("int mx_a(mx_dims_t d, void *stream);", ("mx_a", "mx_dims_t d")),
    ("int mx_a(const float *x, ...);", ("mx_a", "...")),
    ("int mx_a(float x[4]);", ("mx_a", "float x[4]")),
    ("int mx_a(unsigned long long seed);", ("mx_a", "unsigned long long seed")),
    ("int mx_ok(void);\nint mx_a(void (*done)(int), void *stream);", ("mx_a",)),    # not a plain declaration: named, not skipped
    ("int mx_ok(void);\nint64_t mx_a(void);", ("mx_a",)),
    ("int mx_a(void);\nint mx_a(float *x);", ("mx_a",)),
    ("", ()),
    ("/* int mx_a(void); */\n#define MX_OK 0\n", ()),
], ids=["size_t", "int", "struct", "typedef", "variadic", "array", "unsigned", "function-pointer", "return-type", "twice",
        "empty", "no-declaration"])
def test_parser_refuses_what_it_cannot_bind(text, named):
    """Strict: a parameter outside the seven kinds, a declaration of another form, or a text without declarations raises
    ``HipLibraryError`` that names the entry point and the parameter -- nothing is guessed and nothing is skipped."""
    from mod_extraction_amd import _hip
    with pytest.raises(_hip.HipLibraryError) as e:
        _hip.parse_signatures(text)
    for word in named:
        assert word in str(e.value), str(e.value)


def test_missing_header_is_an_error(monkeypatch, tmp_path):
    from mod_extraction_amd import _hip
    monkeypatch.setattr(_hip, "HEADER", str(tmp_path / "modex_hip.h"))
    with pytest.raises(_hip.HipLibraryError, match="modex_hip.h"):
        _hip._header_text()


def test_a_stale_library_is_named(monkeypatch, so_path):
    """A library that lacks a declared symbol (the ABI number cannot tell an added entry point): ``load()``, which reads the
    table as a module attribute at call time, names the symbol and the header and says how to rebuild."""
    from mod_extraction_amd import _hip
    monkeypatch.setattr(_hip, "_lib", None)
    monkeypatch.setattr(_hip, "SIGNATURES", dict(_hip.SIGNATURES, mx_entry_of_tomorrow=[ctypes.c_void_p]))
    with pytest.raises(_hip.HipLibraryError,
                       match=r"mx_entry_of_tomorrow.*include/modex_hip\.h.*rebuild.*python -m mod_extraction_amd\.build"):
        _hip.load()
    monkeypatch.undo()
    assert _hip.load() is not None


def test_the_build_sees_the_header(monkeypatch, so_path):
    """build.py runs nothing when everything is up to date, and compiles every source again and relinks when
    include/modex_hip.h is newer than the objects."""
    from mod_extraction_amd import build
    ran = []
    monkeypatch.setattr(build.subprocess, "check_call", lambda cmd: ran.append(cmd))
    build.build(verbose=False)                                                # so_path built for real: up to date
    assert ran == []
    real = os.path.getmtime
    hdr = os.path.join(build.INCLUDE, "modex_hip.h")
    monkeypatch.setattr(build.os.path, "getmtime", lambda p: 4e9 if os.path.samefile(p, hdr) else real(p))
    build.build(verbose=False)
    compiled = {os.path.basename(c[c.index("-c") + 1]) for c in ran if "-c" in c}
    assert compiled == set(build.sources()) and {"fir_match.hip", "lfo_stitch.hip"} <= compiled
    assert any("-shared" in c for c in ran)


def test_product_has_no_cpu_fallback():
    import torch
    from mod_extraction_amd import _hip, fx
    with pytest.raises(_hip.HipLibraryError):
        fx.MonoFlangerChorusModule(1, 1, 64, 44100, 1.0, 10.0)(torch.zeros(1, 1, 64), torch.zeros(1, 64))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "mod_extraction_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(d, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
                assert "liboracle_ref" not in src, f


def test_library_reads_no_environment():
    """abi.hip: every entry point is a function of its arguments and the stream -- no source of the library calls getenv."""
    csrc = os.path.join(ROOT, "mod_extraction_amd", "csrc")
    seen = 0
    for d, _, files in os.walk(csrc):
        for f in files:
            if f.endswith((".hip", ".h")):
                seen += 1
                assert "getenv" not in open(os.path.join(d, f)).read(), f
    assert seen >= 10


def test_entry_points_reject_bad_arguments_before_touching_the_device(so_path):
    """Every entry point validates its arguments first and returns MX_ERR_ARG / MX_ERR_UNSUPPORTED (never throws, never
    launches): NULL pointers and non-positive sizes are refused here on a box without a GPU."""
    from mod_extraction_amd import _hip
    lib = _hip.load()
    zeros = {ctypes.c_void_p: None, ctypes.c_int64: 0, ctypes.c_int32: 0, ctypes.c_float: 0.0, ctypes.c_double: 0.0,
             ctypes.c_uint64: 0, ctypes.c_uint32: 0}
    skip = {"mx_abi_version"}
    assert len(_hip.SIGNATURES) == N_ENTRY_POINTS
    checked = 0
    for name, argtypes in _hip.SIGNATURES.items():
        if name in skip:
            continue
        rc = getattr(lib, name)(*[zeros[t] for t in argtypes])
        assert rc in (-1, -2), (name, rc)                     # MX_ERR_ARG or MX_ERR_UNSUPPORTED
        checked += 1
    assert checked == N_ENTRY_POINTS - 1 == 123

"""ctypes binding of libmodex_hip.so (the C ABI declared in include/modex_hip.h; the argtypes are derived from its text).

No fallback: if the shared library is missing, or a call returns a non-zero status, this raises.
Device pointers are borrowed from torch tensors; launches go to torch's current HIP stream.
"""
import ctypes
import os
import re
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# MODEX_HIP_LIB: load another build of the same library (kernel experiments); there is no non-HIP fallback
SO_PATH = os.environ.get("MODEX_HIP_LIB") or os.path.join(_HERE, "_lib", "libmodex_hip.so")
ABI_VERSION = 21

_ERR = {-1: "MX_ERR_ARG (bad argument)", -2: "MX_ERR_UNSUPPORTED (size not supported)",
        -3: "MX_ERR_LAUNCH (HIP launch error)"}

HEADER = os.path.join(_HERE, "..", "include", "modex_hip.h")      # where build.py finds it too
# K23's entry points are declared beside their kernels until they are folded into modex_hip.h with an ABI number
HEADER_TRACK = os.path.join(_HERE, "csrc", "track_fit_abi.h")
# K24's likewise
HEADER_RESAMPLE = os.path.join(_HERE, "csrc", "resample_abi.h")
# K25's likewise
HEADER_RATE = os.path.join(_HERE, "csrc", "rate_track_abi.h")
# K26's likewise
HEADER_WARP = os.path.join(_HERE, "csrc", "warp_abi.h")
# K27's likewise
HEADER_SHAPER = os.path.join(_HERE, "csrc", "shaper_match_abi.h")

# the parameter kinds of the C ABI: any pointer, and these six scalars (modex_hip.h states the rule)
_SCALARS = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32,
            "float": ctypes.c_float, "double": ctypes.c_double}


class HipLibraryError(RuntimeError):
    pass


def parse_signatures(text: str) -> dict:
    """name -> argtypes of every ``int mx_name(params);`` that the text of a C header declares, in its order.

    Strict, since a wrong ctypes row corrupts a launch silently: a parameter that is neither a pointer nor one of the six
    scalar types (plain ``int``, ``size_t``, a struct by value, an array, ``...``) raises, and so does a ``mx_name(`` that is
    not such a declaration, a name declared twice, or a text without declarations."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    out = {}
    for name, params in re.findall(r"\bint\s+(mx_\w+)\s*\(([^()]*)\)\s*;", text):
        params = params.strip()
        out[name] = argtypes = []
        for p in ([] if params in ("", "void") else params.split(",")):
            scalar = re.fullmatch(r"\s*(?:const\s+)?(\w+)(?:\s+[A-Za-z_]\w*)?\s*", p)       # `type` or `type name`
            if "*" in p:
                argtypes.append(ctypes.c_void_p)
            elif scalar and scalar.group(1) in _SCALARS:
                argtypes.append(_SCALARS[scalar.group(1)])
            else:
                raise HipLibraryError(f"{name}: parameter `{' '.join(p.split())}` is neither a pointer nor one of "
                                      f"{', '.join(_SCALARS)}; the binding cannot be derived")
    seen = re.findall(r"\b(mx_\w+)\s*\(", text)
    if not out:
        raise HipLibraryError("the header text declares no `int mx_name(...);` entry point")
    if seen != list(out):
        odd = sorted(n for n in set(seen) if n not in out or seen.count(n) > 1)
        raise HipLibraryError(f"not declared exactly once as `int mx_name(params);`: {', '.join(odd)}")
    return out


def _header_text(path: Optional[str] = None) -> str:
    path = HEADER if path is None else path
    if not os.path.isfile(path):
        raise HipLibraryError(f"{path} not found: the ctypes binding is derived from it (there is no other table)")
    with open(path) as f:
        return f.read()


# name -> argtypes of every entry point, derived from include/modex_hip.h (the definitions are compiled against the same text)
SIGNATURES = parse_signatures(_header_text())
# the second table: the entry points of csrc/track_fit_abi.h (mx_track_fit*), bound by load() like the first
SIGNATURES_TRACK = parse_signatures(_header_text(HEADER_TRACK))
TRACK_FIT_ROW_TILE = int(re.search(r"#define\s+MX_TRACK_FIT_ROW_TILE\s+(\d+)", _header_text(HEADER_TRACK)).group(1))
# the third table: the entry points of csrc/resample_abi.h (mx_resample_*)
SIGNATURES_RESAMPLE = parse_signatures(_header_text(HEADER_RESAMPLE))
RESAMPLE_OUT_TILE = int(re.search(r"#define\s+MX_RESAMPLE_OUT_TILE\s+(\d+)", _header_text(HEADER_RESAMPLE)).group(1))
# the fourth table: the entry points of csrc/rate_track_abi.h (mx_rate_track_*), and the limits that header defines
SIGNATURES_RATE = parse_signatures(_header_text(HEADER_RATE))
RATE_TRACK_LIMITS = {k: int(v) for k, v in re.findall(r"#define\s+MX_RATE_TRACK_(\w+)\s+(\d+)\s*$", _header_text(HEADER_RATE),
                                                      flags=re.M)}
# the fifth table: the entry points of csrc/warp_abi.h (mx_warp_*), and that header's limits
SIGNATURES_WARP = parse_signatures(_header_text(HEADER_WARP))
WARP_OUT_TILE = int(re.search(r"#define\s+MX_WARP_OUT_TILE\s+(\d+)", _header_text(HEADER_WARP)).group(1))
WARP_MAX_DRIFT = float(re.search(r"#define\s+MX_WARP_MAX_DRIFT\s+(\S+)", _header_text(HEADER_WARP)).group(1))
WARP_MAX_OFFSET = float(re.search(r"#define\s+MX_WARP_MAX_OFFSET\s+(\S+)", _header_text(HEADER_WARP)).group(1))
# the sixth table: the entry points of csrc/shaper_match_abi.h (mx_shaper_match_*), and that header's limits
SIGNATURES_SHAPER = parse_signatures(_header_text(HEADER_SHAPER))
SHAPER_CHUNK = int(re.search(r"#define\s+MX_SHAPER_CHUNK\s+(\d+)", _header_text(HEADER_SHAPER)).group(1))
SHAPER_MAX_ORDER = int(re.search(r"#define\s+MX_SHAPER_MAX_ORDER\s+(\d+)", _header_text(HEADER_SHAPER)).group(1))

# measurement twins (same signatures): the dependent chain of the sample-recurrent kernels without global traffic
PROBE_TWINS = ("mx_flanger_fwd", "mx_phaser_fwd", "mx_lstm_fwd", "mx_lstm_bwd_l1")

_lib: Optional[ctypes.CDLL] = None


def load() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.isfile(SO_PATH):
            raise HipLibraryError(
                f"{SO_PATH} not found: build it with `python -m mod_extraction_amd.build` "
                "(there is no CPU fallback)")
        lib = ctypes.CDLL(SO_PATH)
        # the tables are read as module attributes here, at call time
        for table, header in ((SIGNATURES, "include/modex_hip.h"), (SIGNATURES_TRACK, "csrc/track_fit_abi.h"),
                              (SIGNATURES_RESAMPLE, "csrc/resample_abi.h"), (SIGNATURES_RATE, "csrc/rate_track_abi.h"),
                              (SIGNATURES_WARP, "csrc/warp_abi.h"), (SIGNATURES_SHAPER, "csrc/shaper_match_abi.h")):
            for name, argtypes in table.items():
                fn = getattr(lib, name, None)
                if fn is None:              # the ABI number does not cover an added entry point: name what a stale build lacks
                    raise HipLibraryError(f"{SO_PATH} has no symbol {name} (declared in {header}): a stale build; "
                                          "rebuild it with `python -m mod_extraction_amd.build`")
                fn.argtypes = argtypes
                fn.restype = ctypes.c_int
        if lib.mx_abi_version() != ABI_VERSION:
            raise HipLibraryError(f"ABI mismatch: library {lib.mx_abi_version()} != binding {ABI_VERSION}")
        _lib = lib
    return _lib


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """Device pointer of a contiguous CUDA(HIP) tensor, or NULL for None."""
    if t is None:
        return None
    if not t.is_cuda:
        raise HipLibraryError("mod_extraction_amd ops need tensors on a HIP device (no CPU fallback)")
    if not t.is_contiguous():
        raise HipLibraryError("non-contiguous tensor passed to a HIP kernel")
    return t.data_ptr()


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class KernelTimer:
    """Optional per-entry-point device timing with HIP events on the launch stream (bench.py).

    ``with KernelTimer({"mx_conv_block_fwd"}) as kt: ...`` records an event pair around every call of
    the selected C-ABI entry points (they launch on torch's current stream, so ``torch.cuda.Event``
    brackets exactly the kernel(s) of that call); ``kt.results()`` synchronises and returns
    ``{tag: [ms, ...]}`` where tag = ``name`` or ``name#<key>`` if ``key_fn(name, args)`` is given."""

    active: Optional["KernelTimer"] = None

    def __init__(self, names, key_fn=None) -> None:
        self.names, self.key_fn = set(names), key_fn
        self.pairs = []

    def __enter__(self) -> "KernelTimer":
        KernelTimer.active = self
        return self

    def __exit__(self, *exc) -> None:
        KernelTimer.active = None

    def results(self):
        torch.cuda.synchronize()
        out = {}
        for tag, a, b in self.pairs:
            out.setdefault(tag, []).append(a.elapsed_time(b))
        return out


class probe_twins:
    """bench.py / tools only: inside this context the four sample-recurrent entry points are routed to their
    ``*_probe`` twins (serial-floor measurement; results are meaningless).  Host-side routing of THIS binding -- the
    shared library itself has no mode switch."""
    on = False

    def __enter__(self):
        probe_twins.on = True
        return self

    def __exit__(self, *exc):
        probe_twins.on = False


def call(name: str, *args) -> None:
    kt = KernelTimer.active
    if probe_twins.on and name in PROBE_TWINS:
        fn_name = name + "_probe"
    else:
        fn_name = name
    if kt is not None and name in kt.names:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = getattr(load(), fn_name)(*args)
        b.record()
        kt.pairs.append((name if kt.key_fn is None else f"{name}#{kt.key_fn(name, args)}", a, b))
    else:
        rc = getattr(load(), fn_name)(*args)
    if rc != 0:
        raise HipLibraryError(f"{name} failed: {_ERR.get(rc, rc)}")

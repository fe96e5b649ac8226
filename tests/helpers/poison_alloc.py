"""Poisoned allocation for tests/test_gpu_uninit_independence.py: inside ``poisoned(pattern)`` every tensor that comes
from ``torch.empty`` / ``torch.empty_like`` / ``torch.empty_strided`` / ``Tensor.new_empty`` (with ``also_zeros=True`` also from
``torch.zeros`` / ``torch.zeros_like`` / ``Tensor.new_zeros``) is filled with a known pattern before its caller sees it, so a
kernel that reads a word nobody wrote, or adds into an output it should overwrite, gives results that differ between patterns.

The fill is an ordinary ``fill_`` on the current stream, i.e. ordered before every kernel the caller launches on the buffer.
Only tensors on the HIP device are filled unless ``any_device=True`` (the helper's own CPU test).

Patterns (every value is in range for anything that might be used as an index, a count or a position: an uninitialised
index word that IS read must show as a difference, not as a wild address):

    pattern   floating types   integer types   bool
    A         0.0              0               untouched
    B         0.5              1               untouched
    C         NaN              1               untouched

``B`` exists beside ``C`` because fminf / fmaxf swallow NaN.  Complex tensors are left alone like bool.

``ctx.sites`` counts the poisoned allocations per call site, keyed ``"<module>:<function>"`` of the frame that called the
allocator (``mod_extraction_amd.models:_f32``, ``mod_extraction_amd.fx:flanger_forward``, ...; a comprehension, generator
expression or lambda counts for the function that runs it).  ``ctx.lines`` is the same table with the line number appended.
"""
import sys
from collections import Counter

import torch

PATTERNS = {"A": (0.0, 0), "B": (0.5, 1), "C": (float("nan"), 1)}
_INT_TYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)
_EMPTY = ((torch, "empty"), (torch, "empty_like"), (torch, "empty_strided"), (torch.Tensor, "new_empty"))
_ZEROS = ((torch, "zeros"), (torch, "zeros_like"), (torch.Tensor, "new_zeros"))


def poison_value(pattern: str, dtype: torch.dtype):
    """The fill value of ``pattern`` for ``dtype``, or None for the types the patterns leave untouched."""
    fl, it = PATTERNS[pattern]
    if dtype.is_floating_point:
        return fl
    if dtype in _INT_TYPES:
        return it
    return None


class poisoned:
    """Context manager; see the module docstring.  Not re-entrant."""

    def __init__(self, pattern: str, also_zeros: bool = False, any_device: bool = False) -> None:
        if pattern not in PATTERNS:
            raise ValueError(f"unknown poison pattern {pattern!r}")
        self.pattern, self.also_zeros, self.any_device = pattern, also_zeros, any_device
        self.sites = Counter()
        self.lines = Counter()                   # the same allocations keyed "<module>:<function>:<line>"
        self._saved = []

    # ---- the call-site table ----------------------------------------------------------------------------------------
    @property
    def total(self) -> int:
        return sum(self.sites.values())

    def functions(self, module_suffix: str = "") -> set:
        """The functions named by the table ("module:function" keys), optionally only those of modules ending in the suffix."""
        return {k for k in self.sites if k.split(":")[0].endswith(module_suffix)}

    # ---- patching ---------------------------------------------------------------------------------------------------
    def _wrap(self, orig):
        ctx = self

        def alloc(*args, **kwargs):
            t = orig(*args, **kwargs)
            if not isinstance(t, torch.Tensor) or t.numel() == 0:
                return t
            if t.device.type != "cuda" and not (ctx.any_device and t.device.type == "cpu"):
                return t
            v = poison_value(ctx.pattern, t.dtype)
            if v is None:
                return t
            with torch.no_grad():
                t.fill_(v)
            f = sys._getframe(1)
            while f.f_code.co_name.startswith("<") and f.f_back is not None:      # <listcomp>, <genexpr>, <lambda>: the function around it
                f = f.f_back
            site = f"{f.f_globals.get('__name__', '?')}:{f.f_code.co_name}"
            ctx.sites[site] += 1
            ctx.lines[f"{site}:{f.f_lineno}"] += 1
            return t

        alloc.__name__ = getattr(orig, "__name__", "alloc")
        alloc.__wrapped__ = orig
        return alloc

    def __enter__(self):
        assert not self._saved, "poisoned() is not re-entrant"
        try:
            for owner, name in _EMPTY + (_ZEROS if self.also_zeros else ()):
                orig = getattr(owner, name)
                self._saved.append((owner, name, orig, name in vars(owner)))
                setattr(owner, name, self._wrap(orig))
        except BaseException:
            self._restore()
            raise
        return self

    def _restore(self) -> None:
        while self._saved:
            owner, name, orig, own = self._saved.pop()
            if own:
                setattr(owner, name, orig)
            else:                                # inherited (Tensor.new_empty lives on the C base class): drop the shadow
                delattr(owner, name)

    def __exit__(self, *exc) -> bool:
        self._restore()
        return False

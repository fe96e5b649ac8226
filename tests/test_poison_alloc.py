"""tests/helpers/poison_alloc.py on the CPU (device filter off): every patched allocator returns the pattern for every dtype
of the table, the originals come back (also when the body raises), ``also_zeros=False`` leaves torch.zeros alone, and the
call-site table names the caller."""
import math

import pytest
import torch

from tests.helpers.poison_alloc import PATTERNS, poison_value, poisoned

FLOATS = (torch.float16, torch.float32, torch.float64)
INTS = (torch.uint8, torch.int16, torch.int32, torch.int64)
NAMES = ("empty", "empty_like", "empty_strided", "zeros", "zeros_like")


def _originals():
    return [getattr(torch, n) for n in NAMES] + [torch.Tensor.new_empty, torch.Tensor.new_zeros]


def _allocators(also_zeros):
    """name -> callable(dtype) that allocates 3 x 5 elements through the patched attribute (looked up at call time)."""
    a = {"empty": lambda dt: torch.empty(3, 5, dtype=dt),
         "empty_kw": lambda dt: torch.empty((3, 5), dtype=dt, device="cpu"),
         "empty_like": lambda dt: torch.empty_like(torch.ones(3, 5, dtype=dt)),
         "empty_strided": lambda dt: torch.empty_strided((3, 5), (8, 1), dtype=dt),
         "new_empty": lambda dt: torch.ones(2, dtype=dt).new_empty((3, 5))}
    if also_zeros:
        a.update({"zeros": lambda dt: torch.zeros(3, 5, dtype=dt),
                  "zeros_like": lambda dt: torch.zeros_like(torch.ones(3, 5, dtype=dt)),
                  "new_zeros": lambda dt: torch.ones(2, dtype=dt).new_zeros((3, 5))})
    return a


def _holds(t, v):
    if isinstance(v, float) and math.isnan(v):
        return bool(torch.isnan(t).all())
    return bool((t == v).all())


@pytest.mark.parametrize("pattern", ["A", "B", "C"])
@pytest.mark.parametrize("also_zeros", [False, True])
def test_every_allocator_returns_the_pattern_for_every_dtype(pattern, also_zeros):
    fl, it = PATTERNS[pattern]
    with poisoned(pattern, also_zeros=also_zeros, any_device=True) as ctx:
        for name, alloc in _allocators(also_zeros).items():
            for dt in FLOATS:
                t = alloc(dt)
                assert t.dtype == dt and t.shape == (3, 5) and _holds(t, fl), (name, dt)
            for dt in INTS:
                t = alloc(dt)
                assert t.dtype == dt and t.shape == (3, 5) and _holds(t, it), (name, dt)
        n_alloc = len(_allocators(also_zeros)) * (len(FLOATS) + len(INTS))
        assert ctx.total == n_alloc


def test_pattern_values_are_the_documented_ones():
    assert set(PATTERNS) == {"A", "B", "C"}
    assert PATTERNS["A"] == (0.0, 0) and PATTERNS["B"] == (0.5, 1)
    assert math.isnan(PATTERNS["C"][0]) and PATTERNS["C"][1] == 1


def test_bool_is_left_untouched_and_not_counted():
    with poisoned("B", also_zeros=True, any_device=True) as ctx:
        assert not torch.zeros(4, dtype=torch.bool).any()
        torch.empty(4, dtype=torch.bool)
        assert ctx.total == 0
    assert poison_value("C", torch.bool) is None


def test_device_filter_leaves_cpu_tensors_alone_by_default():
    with poisoned("B", also_zeros=True) as ctx:
        assert _holds(torch.zeros(7), 0.0)
        torch.empty(7)
        assert ctx.total == 0


def test_originals_are_restored_after_the_context():
    before = _originals()
    own = "new_empty" in vars(torch.Tensor), "new_zeros" in vars(torch.Tensor)
    with poisoned("C", also_zeros=True, any_device=True):
        inside = _originals()
        assert all(a is not b for a, b in zip(before, inside))
    assert all(a is b for a, b in zip(before, _originals()))
    assert own == ("new_empty" in vars(torch.Tensor), "new_zeros" in vars(torch.Tensor))
    assert _holds(torch.zeros(3), 0.0)


def test_originals_are_restored_when_the_body_raises():
    before = _originals()
    with pytest.raises(RuntimeError, match="from the body"):
        with poisoned("B", also_zeros=True, any_device=True):
            assert _holds(torch.empty(3), 0.5)
            raise RuntimeError("from the body")
    assert all(a is b for a, b in zip(before, _originals()))
    assert _holds(torch.zeros(3), 0.0)


def test_also_zeros_false_leaves_zeros_alone():
    zeros, zeros_like, new_zeros = torch.zeros, torch.zeros_like, torch.Tensor.new_zeros
    with poisoned("B", any_device=True) as ctx:
        assert torch.zeros is zeros and torch.zeros_like is zeros_like and torch.Tensor.new_zeros is new_zeros
        assert _holds(torch.zeros(5), 0.0) and _holds(torch.zeros_like(torch.ones(5)), 0.0)
        assert _holds(torch.ones(2).new_zeros(5), 0.0)
        assert ctx.total == 0
        assert _holds(torch.empty(5), 0.5)


def _some_wrapper(n):
    return torch.empty(n), torch.ones(n, dtype=torch.int32).new_empty(n)


def _comprehension_wrapper(n):
    return [torch.empty(n) for _ in range(3)], tuple(torch.empty(n) for _ in range(2))


def test_call_site_table_names_the_caller():
    with poisoned("B", any_device=True) as ctx:
        _some_wrapper(4)
        _some_wrapper(4)
        torch.empty_like(torch.ones(2))
        _comprehension_wrapper(2)
    assert ctx.sites[f"{__name__}:_some_wrapper"] == 4
    assert ctx.sites[f"{__name__}:test_call_site_table_names_the_caller"] == 1
    assert ctx.sites[f"{__name__}:_comprehension_wrapper"] == 5           # not "<listcomp>" / "<genexpr>"
    assert ctx.total == 10 and sum(ctx.lines.values()) == 10
    assert all(k.rsplit(":", 1)[0] in ctx.sites and k.rsplit(":", 1)[1].isdigit() for k in ctx.lines)
    assert ctx.functions("test_poison_alloc") == {f"{__name__}:_some_wrapper", f"{__name__}:_comprehension_wrapper",
                                                  f"{__name__}:test_call_site_table_names_the_caller"}


def test_requires_grad_and_unknown_pattern():
    with poisoned("B", any_device=True):
        t = torch.empty(3, requires_grad=True)            # the fill must not trip autograd's leaf check
        assert t.requires_grad and t.is_leaf and _holds(t.detach(), 0.5)
    with pytest.raises(ValueError):
        poisoned("D")

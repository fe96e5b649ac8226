"""GPU: mx_effect_loss_sums and mx_effect_loss_grad (csrc/effect_loss.hip) on their raw entry points, held per clip and per
element to the fp64 references and the derived rounding bounds of tests/helpers/effect_loss64.py.  The step tests of the
audio-loss family use ``effect_loss_grad`` as their oracle; this file is what holds that oracle.

Conventions of tests/test_gpu_midblock_units.py: every output is an ``Out`` between two guard bands, body and guards pre-filled
with a NaN bit pattern that must survive; prediction and target are rows of buffers with a stride of T or T + 3 (chosen
independently), the pad columns holding 1e30; the gradient has a stride of T or T + 5 and its pad columns must keep the sentinel;
every gate is ``worst ratio to its bound <= tol`` with tol = 1.0, per clip.

Batches (tests/helpers/effect_loss64.py::KINDS_BY_B): an ordinary clip whose every fifth sample has prediction == target, a silent
target (B >= 2), a clip with prediction = target + 0.3, an all-equal clip.

Measured on the MI355X, worst ratio over all shapes (tol = 1.0): sums |e| 0.45, e^2 0.19, t^2 0.48, e 0.30; gradient without
accumulate l1 0.12, mse 0.31, esr 0.32, dc 0.23, mix 0.38; with accumulate 0.998 (one rounding of o + g: its error reaches
u |o + g| whenever the sum lands just above a power of two, which is the whole of that bound); the four scalars of
effect_loss_terms 0.13, 0.07, 0.08, 0.15.  tests/test_effect_loss64.py shows on the CPU that six seeded coefficient defects leave
the bound on every clip.
"""
import numpy as np
import pytest
import torch

from tests.helpers import effect_loss64 as E
from tests.helpers.gpu_harness import ARG, POISON, SENT, Out, bits, call, dv, f32, f64, ratio, status

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (1, 63), (1, 64), (2, 65), (3, 255), (2, 256), (3, 257), (2, 1000), (1, 4097)]
WEIGHTS = {"l1": (1.0, 0.0, 0.0, 0.0), "mse": (0.0, 1.0, 0.0, 0.0), "esr": (0.0, 0.0, 1.0, 0.0), "dc": (0.0, 0.0, 0.0, 1.0),
           "mix": (0.3, 0.7, 0.4, 2.0)}
EPS = (1e-8, 1e-3)


def _rows_in(dev, a, stride):
    """(B, T) as rows of a (B, stride) buffer whose pad columns hold 1e30."""
    B, T = a.shape
    buf = np.full((B, stride), POISON, f32)
    buf[:, :T] = a
    return dv(dev, buf)


def _batches(B, T):
    for v, kinds in enumerate(E.KINDS_BY_B[B]):
        a, t = E.clips(kinds, T, 1000 * T + 10 * B + v)
        yield kinds, a, t


def _layouts(dev, a, t):
    """Prediction and target at the strides T and T + 3, independently: ((a_dev, a_stride), (t_dev, t_stride)) four times."""
    T = a.shape[1]
    ad = {s: _rows_in(dev, a, s) for s in (T, T + 3)}
    td = {s: _rows_in(dev, t, s) for s in (T, T + 3)}
    return [((ad[sa], sa), (td[st], st)) for sa in (T, T + 3) for st in (T, T + 3)]


@pytest.mark.parametrize("B,T", SHAPES)
def test_sums_per_clip(dev, B, T):
    """Every clip's four sums against fp64, never averaged: sum |e| within 2 u S_abs, sum e^2 within 4 u S_sq, sum t^2 within
    2 u S_tt, sum e within u S_abs + 2 u |S_e| (u = 2^-24).  The all-equal clip's three error sums and the silent clip's
    sum t^2 have a zero bound: they must be exactly 0."""
    tol = 1.0
    worst = np.zeros(4)
    for kinds, a, t in _batches(B, T):
        ref, bound = E.sums64(a, t)
        for (ad, sa), (td, st) in _layouts(dev, a, t):
            part = Out(dev, B * 4)
            call("mx_effect_loss_sums", ad, sa, td, st, B, T, part)
            assert part.guards_intact() and part.untouched() == 0
            got = part.read().reshape(B, 4)
            for b, kind in enumerate(kinds):
                r = [ratio(got[b, k], ref[b, k], bound[b, k]) for k in range(4)]
                worst = np.maximum(worst, r)
                assert r[0] <= tol, (kind, b, sa, st)
                assert r[1] <= tol, (kind, b, sa, st)
                assert r[2] <= tol, (kind, b, sa, st)
                assert r[3] <= tol, (kind, b, sa, st)
                if kind == "equal":
                    assert not got[b, [0, 1, 3]].any()
                if kind == "silent":
                    assert got[b, 2] == 0.0
    print(f"[measured] effect_loss_sums {B}x{T}: worst ratio abs {worst[0]:.3f} sq {worst[1]:.3f} tt {worst[2]:.3f} e {worst[3]:.3f}")


@pytest.mark.parametrize("name", list(WEIGHTS))
@pytest.mark.parametrize("B,T", SHAPES)
def test_grad_per_element(dev, B, T, name):
    """Every element within 8 u (|c_l1| [d != 0] + (|c_mse| + |c_esr|) |d| + |c_dc|), with accumulate = 1 plus u (|o| + |g|) on a
    random previous content o; eps = 1e-8 and 1e-3 (at 1e-3 an eps added to the wrong one of sum t^2 / mean t^2 moves a loud
    clip's coefficient by far more than the bound); dy_stride T and T + 5, the pad columns keep the sentinel.  The all-equal clip
    gets exactly 0 from l1, mse and esr (and exactly o with accumulate = 1)."""
    tol = 1.0
    w = WEIGHTS[name]
    worst = {}
    for v, (kinds, a, t) in enumerate(_batches(B, T)):
        layouts = _layouts(dev, a, t)
        prev = np.random.default_rng(T + v).standard_normal((B, T)).astype(f32)
        for eps in EPS:
            for accumulate in (0, 1):
                ref = E.grad64(a, t, B, *w, eps, prev=prev if accumulate else None)
                for (ad, sa), (td, st) in layouts:
                    for ds in (T, T + 5):
                        init = np.full((B, ds), SENT, np.int32).view(f32)
                        if accumulate:
                            init[:, :T] = prev
                        dy = Out(dev, B * ds, init=init)
                        call("mx_effect_loss_grad", ad, sa, td, st, B, T, *w, eps, accumulate, dy, ds)
                        body = dy.read().reshape(B, ds)
                        assert dy.guards_intact() and dy.untouched() == B * (ds - T)
                        assert (bits(body[:, T:]) == np.int32(SENT)).all()
                        got = body[:, :T]
                        for b, kind in enumerate(kinds):
                            r = ratio(got[b], ref["grad"][b], ref["bound"][b])
                            key = kind + ("+o" if accumulate else "")
                            worst[key] = max(worst.get(key, 0.0), r)
                            assert r <= tol, (kind, b, eps, accumulate, sa, st, ds)
                            if kind == "equal" and name != "dc":
                                assert np.array_equal(got[b], prev[b] if accumulate else np.zeros(T, f32))
    print(f"[measured] effect_loss_grad {name} {B}x{T}: worst ratio", {k: round(x, 3) for k, x in worst.items()})


def test_terms_make_every_clip_count(dev):
    """effect_loss_terms on a batch without a silent clip (B = 2, T = 256), against the fp64 mean of the per-clip ratios: the error
    the sums' bounds allow, carried through the ratios, plus 4 u of the value for the fp32 arithmetic behind the sums -- with
    B = 2 and T = 256 every division by B, T or B T is exact, which leaves at most: l1 / mse one add; esr one add of eps, one
    division, one add; dc one square, one add of eps, one division, one add."""
    from mod_extraction_amd.effect_losses import effect_loss_terms
    B, T, eps = 2, 256, 1e-3
    a, t = E.clips(("ordinary", "dc"), T, 77)
    got = effect_loss_terms(dv(dev, a)[:, None, :], dv(dev, t)[:, None, :], eps=eps)
    want = E.terms64(a, t, eps)
    tol = 1.0
    for k in ("l1", "mse", "esr", "dc"):
        value, carried = want[k]
        r = ratio(float(got[k]), value, carried + 4 * E.U24 * abs(value))
        print(f"[measured] effect_loss_terms {k}: ratio {r:.3f} value {value:.6g}")
        assert r <= tol, k
    # every clip counts: the scalar without the quieter clip's share is far outside the bound
    s, _ = E.sums64(a, t)
    per_clip = s[:, 1] / (s[:, 2] + f64(f32(eps)))
    assert per_clip.min() / B > 1e3 * (want["esr"][1] + 4 * E.U24 * want["esr"][0])


def test_argument_statuses(dev):
    """Null pointers, B <= 0, T <= 0 and (gradient) dy_stride < T -> MX_ERR_ARG, before any launch: the outputs keep every sentinel."""
    B, T = 2, 8
    a, t = E.clips(("ordinary", "dc"), T, 1)
    ad, td = dv(dev, a), dv(dev, t)
    part, dy = Out(dev, B * 4), Out(dev, B * T)
    ok = {"mx_effect_loss_sums": [ad, T, td, T, B, T, part],
          "mx_effect_loss_grad": [ad, T, td, T, B, T, 1.0, 1.0, 1.0, 1.0, 1e-8, 0, dy, T]}
    ptrs = {"mx_effect_loss_sums": (0, 2, 6), "mx_effect_loss_grad": (0, 2, 12)}
    for name, args in ok.items():
        for i in ptrs[name]:
            assert status(name, *[None if j == i else v for j, v in enumerate(args)]) == ARG, (name, i)
        for i in (4, 5):
            for bad in (0, -1):
                assert status(name, *[bad if j == i else v for j, v in enumerate(args)]) == ARG, (name, i, bad)
    name = "mx_effect_loss_grad"
    assert status(name, *[T - 1 if j == 13 else v for j, v in enumerate(ok[name])]) == ARG
    torch.cuda.synchronize()
    assert part.guards_intact() and part.untouched() == part.words
    assert dy.guards_intact() and dy.untouched() == dy.words

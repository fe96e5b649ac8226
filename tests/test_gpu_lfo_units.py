"""GPU: the oldest kernel family on its raw entry points against the independent references of tests/helpers/lfo_units64.py --
mx_lfo_synth, mx_interp_linear, mx_interp_linear_bwd (lfo.hip, K1), mx_smoothen, mx_find_corners, mx_stretch_corners,
mx_stretch_corners_bwd, mx_check_mod_sig (corners.hip, K9) and mx_lfo_loss (head_loss.hip).  Inputs and sizes:
tests/helpers/lfo_units_cases.py; tests/test_lfo_units64.py holds the references against the oracle and checks the exclusion
caps on the CPU.  Conventions of tests/test_gpu_block1_units.py: outputs between NaN-pattern guard bands, every tolerance gate
``measured <= tol``.

No gate is derived from a kernel's output.  A derived gate is FOUR times the oracle's own fp32 error against the same fp64
reference (the device's cosf / powf / summation order may be a couple of ulp wider than the host's), computed on the CPU by
lfo_units_cases.py when the test runs, never below a floor.  The oracle figures as measured on the CPU (torch 2.x, x86-64):

gate                         | derived from (oracle fp32 vs the fp64 reference)                        | factor, floor | gate
-----------------------------|-------------------------------------------------------------------------|---------------|---------
lfo_synth, exponent 1        | make_mod_signal (+ util resampling): worst |err| 8.96e-08               | 4, 2^-22      | 3.58e-07
lfo_synth, exponent 2        | 1.31e-07                                                                | 4, 2^-22      | 5.24e-07
lfo_synth, exponent 3        | 1.75e-07                                                                | 4, 2^-22      | 7.01e-07
lfo_synth, exponent 0.5      | 1.87e-04 (sqrt of (cos + 1) / 2 near 0 turns one fp32 rounding, 6e-8,   | 4, 2^-22      | 7.49e-04
                             | into its square root)                                                   |               |
lfo_synth, exponent 1.7      | 1.21e-07                                                                | 4, 2^-22      | 4.84e-07
lfo_synth saw / rsaw / tri,  | IEEE basic operations only: lfo_bits32                                  | --            | bit equality
  exponent 1, 2, 3, no resampling                                                                        |               |
interp forward               | two fp32 roundings (the product lam1 x1, the fused sum)                 | --            | 1 ulp of max(|x0|, |x1|)
interp backward              | torch fp32 autograd of F.interpolate, per window, relative to           | 4, 1e-6       | 1e-6 .. 3.4e-06
                             | max |dx_ref|: 0 .. 8.4e-07 (the whole (345, 86410) axis)                |               |
corner maps, stretch,        | IEEE basic operations only                                              | --            | ==
  validity, moving average   |                                                                         |               |
stretch backward             | stretch_corners_torch under fp32 autograd, per row relative to          | 4, 1e-6       | n = 9: 1e-6, 90: 2.2e-06,
                             | max |dx_ref|: n = 9: 2.0e-07, n = 90: 5.5e-07, n = 345: 9.4e-07          |               | 345: 3.8e-06
lfo_loss gradient            | a handful of fp32 roundings of the coefficient arithmetic               | --            | 2^-21 of max |grad_ref|
lfo_loss terms, total (grid) | one fp32 rounding of an fp64 sum, doubled                               | --            | 2^-22 rel., 1e-12 abs.
lfo_loss terms, total        | oracle.losses in fp32: l1 1.3e-07, fdl1 6.9e-07, sdl1 2.8e-06,          | 4, 2^-22      | up to 1.1e-05 (sdl1)
  (generic)                  | mse 1.2e-07, total 1.8e-06 (worst over the cases; used per case)        |               |

Excluded points: lfo_synth points whose decision margin (lfo_value64) is below 1e-5 -- at most 1 % of a launch, asserted; loss
gradient elements of the generic family whose margin is below 1e-6 of the amplitude -- at most 2 %, asserted.
"""
import numpy as np
import pytest

from tests.helpers import lfo_units64 as L
from tests.helpers import lfo_units_cases as C
from tests.helpers.gpu_harness import ARG, UNSUPPORTED, Out, bits, call, dv, f32, f64, ratio, status

pytestmark = pytest.mark.gpu
i32 = np.int32


def _opt(dev, a, dtype):
    return None if a is None else dv(dev, a, dtype)


# ==== mx_lfo_synth =============================================================================================================
_SYNTH_PAIRS = list(dict.fromkeys((c["n_src"], c["n_out"]) for c in C.synth_cases()))


@pytest.mark.parametrize("n_src,n_out", _SYNTH_PAIRS)
def test_lfo_synth(dev, n_src, n_out):
    """Seven rows, one per shape, in one launch; five launches per size pair: the start offset (the phaser's cropped label), the
    pow fast paths and the generic powf, the on-the-fly resampling, null shape / exp / start pointers."""
    gates = C.synth_gates()
    for case in (c for c in C.synth_cases() if (c["n_src"], c["n_out"]) == (n_src, n_out)):
        B = C.SYNTH_B
        out = Out(dev, B * n_out)
        call("mx_lfo_synth", dv(dev, case["freq"]), dv(dev, case["phase"]), _opt(dev, case["shape"], i32), _opt(dev, case["exp"], f32),
             _opt(dev, case["start"], i32), B, n_src, n_out, float(case["sr"]), out)
        got = out.read().reshape(B, n_out)
        assert out.guards_intact(), case["name"]
        ref, margin, args = C.synth_ref(case)
        ok = margin >= C.MARGIN_SYNTH
        assert float((~ok).mean()) <= C.CAP_SYNTH, case["name"]
        for b in range(B):
            sh, e, st = C.synth_row_params(case, b)
            if sh in (L.TRI, L.SAW, L.RSAW) and e in (1.0, 2.0, 3.0) and n_out == n_src:
                want = L.lfo_bits32(args[b], sh, e)
                assert np.array_equal(bits(got[b])[ok[b]], bits(want)[ok[b]]), (case["name"], L.SHAPES[sh], e)
            else:
                tol = gates[float(f32(e))][1]
                err = float(np.abs(got[b].astype(f64) - ref[b])[ok[b]].max()) if ok[b].any() else 0.0
                assert err <= tol, (case["name"], L.SHAPES[sh], e, st)


def test_lfo_synth_status_codes(dev):
    f, out = dv(dev, np.ones(2, f32)), Out(dev, 16)
    assert status("mx_lfo_synth", None, f, None, None, None, 2, 8, 8, 441.0, out) == ARG
    assert status("mx_lfo_synth", f, f, None, None, None, 0, 8, 8, 441.0, out) == ARG
    assert status("mx_lfo_synth", f, f, None, None, None, 2, 0, 8, 441.0, out) == ARG
    assert status("mx_lfo_synth", f, f, None, None, None, 2, 8, 8, 0.0, out) == ARG
    assert status("mx_lfo_synth", f, f, None, None, None, 2, 1 << 29, 8, 441.0, out) == UNSUPPORTED
    assert out.untouched() == out.words and out.guards_intact()


# ==== mx_interp_linear / mx_interp_linear_bwd ==================================================================================
@pytest.mark.parametrize("n_in,n_out", C.INTERP_PAIRS)
def test_interp_forward(dev, n_in, n_out):
    g = np.random.default_rng(n_in * 7 + n_out)
    x = (g.uniform(-1, 1, (C.INTERP_ROWS, n_in)) * np.array([[1.0], [1e-3], [300.0]])).astype(f32)
    x[:, ::3] = 0
    y = Out(dev, C.INTERP_ROWS * n_out)
    call("mx_interp_linear", dv(dev, x), C.INTERP_ROWS, n_in, n_out, y)
    got = y.read().reshape(C.INTERP_ROWS, n_out)
    assert y.guards_intact()
    i0, i1, _, _ = L.interp_taps32(n_in, n_out)
    bound = np.spacing(np.maximum(np.abs(x[:, i0]), np.abs(x[:, i1])))       # one fp32 ulp of max(|x0|, |x1|)
    tol = 1.0
    assert ratio(got, L.interp64(x, n_in, n_out), bound) <= tol


@pytest.mark.parametrize("n_in,n_out", C.INTERP_PAIRS)
def test_interp_backward(dev, n_in, n_out):
    """Every window, once with dy contiguous and once with dy_stride = j_len + 5, the five pad floats holding 1e30."""
    R = C.INTERP_ROWS
    for name, (j0, j_len) in C.interp_windows(n_in, n_out).items():
        dy = C.interp_dy(n_in, n_out, j0, j_len)
        ref = L.interp_bwd64(dy, n_in, n_out, j0)
        oracle_err, tol = C.interp_bwd_gate(n_in, n_out, j0, j_len)
        results = []
        for stride in (j_len, j_len + 5):
            padded = np.full((R, stride), 1e30, f32)
            padded[:, :j_len] = dy
            dx = Out(dev, R * n_in)
            call("mx_interp_linear_bwd", dv(dev, padded), stride, R, n_in, n_out, j0, j_len, dx)
            got = dx.read().reshape(R, n_in)
            assert dx.guards_intact(), (name, stride)
            err = float(np.abs(got.astype(f64) - ref).max() / np.abs(ref).max())
            assert err <= tol, (name, stride, oracle_err)
            results.append(got)
        assert np.array_equal(bits(results[0]), bits(results[1])), name


# ==== corners.hip ==============================================================================================================
@pytest.mark.parametrize("R", C.CORNER_R)
@pytest.mark.parametrize("n", C.CORNER_N)
def test_corner_maps_and_stretch(dev, n, R):
    """Designed rows (exactly max_n_corners corners and one more, plateaus, a monotone row, map values above 1, equal anchors
    with a gain that is not finite) in one, in a partly filled and in more than one 64-row workgroup."""
    rows, names = C.corner_stack(n, R)
    x = dv(dev, rows)
    top, bot = Out(dev, R * n), Out(dev, R * n)
    call("mx_find_corners", x, R, n, top, bot)
    t_ref, b_ref = L.corners_ref(rows)
    assert top.guards_intact() and bot.guards_intact()
    assert np.array_equal(top.read().reshape(R, n), t_ref) and np.array_equal(bot.read().reshape(R, n), b_ref)
    for mc in C.MAX_N_CORNERS:
        out = Out(dev, R * n)
        call("mx_stretch_corners", x, R, n, mc, out)
        want = L.stretch_ref(rows, mc)
        assert out.guards_intact()
        assert np.array_equal(out.read().reshape(R, n), want, equal_nan=True), mc
        changed = (want != rows).any(1)
        assert changed[0] and changed[R - 1] and (R < 63 or not changed.all())        # copied rows too


@pytest.mark.parametrize("R", C.CORNER_R)
def test_check_mod_sig(dev, R):
    n = 90
    rows, names = C.corner_stack(n, R, C.VALID_ROWS, C.VALID_GOOD_ROW)
    x = dv(dev, rows)
    for args in C.VALID_ARGS:
        want = L.valid_ref(rows, *args)
        if R >= 63:
            assert 0.25 <= float(want.mean()) <= 0.75, args                   # cannot pass vacuously
        assert want[0] == 1 and want[R - 1] == 1
        valid = Out(dev, R, i32)
        call("mx_check_mod_sig", x, R, n, *args, valid)
        assert valid.guards_intact()
        assert np.array_equal(valid.read(), want), args


@pytest.mark.parametrize("R,n,k", C.SMOOTHEN_CASES)
def test_smoothen(dev, R, n, k):
    x = np.random.default_rng(R + 10 * n + k).uniform(0, 1, (R, n)).astype(f32)
    out = Out(dev, R * (n - k + 1))
    call("mx_smoothen", dv(dev, x), R, n, k, out)
    assert out.guards_intact()
    assert np.array_equal(out.read().reshape(R, n - k + 1), L.smoothen_ref(x, k))


@pytest.mark.parametrize("R", C.CORNER_R)
@pytest.mark.parametrize("n", C.CORNER_N)
def test_stretch_backward(dev, n, R):
    rows, names = C.corner_stack(n, R)
    g = C.stretch_dout(n, R)
    x, dout = dv(dev, rows), dv(dev, g)
    for mc in C.MAX_N_CORNERS:
        dx = Out(dev, R * n)
        call("mx_stretch_corners_bwd", x, dout, R, n, mc, dx)
        got = dx.read().reshape(R, n)
        assert dx.guards_intact()
        finite = L.stretch_gain_finite(rows, mc)                             # rows with a gain x / 0 are left out
        assert finite[0] and finite[R - 1]
        ref = L.stretch_bwd64(rows[finite], g[finite], mc)
        oracle_err, tol = C.stretch_bwd_gate(n, mc)
        err = float((np.abs(got[finite].astype(f64) - ref).max(1) / np.abs(ref).max(1)).max())
        assert err <= tol, (mc, oracle_err)
        keep = L.stretch_passthrough(rows, mc) & finite[:, None]
        assert (keep.any() or R < 63) and np.array_equal(bits(got)[keep], bits(g)[keep]), mc     # copied rows, unstretched segments: dout itself


# ==== mx_lfo_loss ==============================================================================================================
def _run_loss(dev, y_hat, y, w, with_grad=True):
    B, n = y_hat.shape
    part, losses, grad = Out(dev, B * 4), Out(dev, 5), Out(dev, B * n)
    call("mx_lfo_loss", dv(dev, y_hat), dv(dev, y), B, n, *[float(v) for v in w], part, losses, grad if with_grad else None)
    assert part.guards_intact() and losses.guards_intact() and grad.guards_intact()
    if not with_grad:
        assert grad.untouched() == grad.words
    return losses.read(), grad.read().reshape(B, n)


@pytest.mark.parametrize("n", C.LOSS_N)
@pytest.mark.parametrize("B", C.LOSS_B)
def test_lfo_loss(dev, B, n):
    """grid: inputs on multiples of 1 / 64 with exact zeros of the error and of its first and second differences -- every sign
    decision is exact, nothing is excluded.  generic: LFO-like rows plus 1e-2 noise at amplitude 1 and 1e-4.  The weights include
    a zero and a negative one: such a term stays out of the total AND of the gradient (lightning.py:48-52)."""
    families = [("grid", 1.0, C.loss_grid_inputs(B, n))] + [("generic", a, C.loss_generic_inputs(B, n, a)) for a in C.LOSS_AMPLITUDES]
    for family, amp, (y_hat, y) in families:
        for wi, w in enumerate(C.LOSS_W):
            ref = L.lfo_loss64(y_hat, y, w)
            losses, grad = _run_loss(dev, y_hat, y, w)
            want = np.append(ref["terms"], ref["total"])
            rel = np.full(5, 2.0 ** -22)
            if family == "generic":
                rel = np.maximum(rel, 4.0 * C.oracle_loss_error(y_hat, y, w))
            tol = 1.0
            assert ratio(losses, want, np.maximum(rel * np.abs(want), 1e-12)) <= tol, (family, amp, w)
            ok = np.ones((B, n), bool)
            if family == "generic":
                ok = ref["margin"] >= C.MARGIN_LOSS * amp
                assert float((~ok).mean()) <= C.CAP_LOSS, (amp, w)
            gmax = float(np.abs(ref["grad"]).max())
            tol = 2.0 ** -21
            assert float(np.abs(grad.astype(f64) - ref["grad"])[ok].max()) / gmax <= tol, (family, amp, w)
            again, grad2 = _run_loss(dev, y_hat, y, w)                        # determinism: the same bits
            assert np.array_equal(bits(again), bits(losses)) and np.array_equal(bits(grad2), bits(grad))
            if wi == 0 and family == "grid":                                 # grad null: values only, the same values
                only, _ = _run_loss(dev, y_hat, y, w, with_grad=False)
                assert np.array_equal(bits(only), bits(losses))


def test_lfo_loss_status_codes(dev):
    z = dv(dev, np.zeros((2, 2049), f32))
    part, losses, grad = Out(dev, 8), Out(dev, 5), Out(dev, 2 * 2049)
    assert status("mx_lfo_loss", z, z, 2, 2049, 1.0, 1.0, 1.0, 1.0, part, losses, grad) == UNSUPPORTED       # LOSS_MAXN = 2048
    assert status("mx_lfo_loss", None, z, 2, 8, 1.0, 1.0, 1.0, 1.0, part, losses, grad) == ARG
    assert status("mx_lfo_loss", z, z, 2, 8, 1.0, 1.0, 1.0, 1.0, None, losses, grad) == ARG
    assert status("mx_lfo_loss", z, z, 0, 8, 1.0, 1.0, 1.0, 1.0, part, losses, grad) == ARG
    assert status("mx_lfo_loss", z, z, 2, 0, 1.0, 1.0, 1.0, 1.0, part, losses, grad) == ARG
    for o in (part, losses, grad):                                           # no launch: nothing was written
        assert o.untouched() == o.words and o.guards_intact()
    assert status("mx_lfo_loss", z, z, 2, 2048, 1.0, 1.0, 1.0, 1.0, part, losses, grad) == 0
    assert float(losses.read()[4]) == 0.0

"""CPU: the references of tests/helpers/lfo_units64.py against the oracle (oracle.modulations, oracle.util, oracle.losses, torch
autograd in float64) on the sizes of tests/test_gpu_lfo_units.py, the designed rows against their listed corners, and the
exclusion caps of every input the GPU file uses.  == where the arithmetic is IEEE-exact (phase, saw / tri, taps, corners,
stretch, validity, moving average), 1e-12 relative where both sides are fp64."""
import math

import numpy as np
import pytest
import torch

from oracle import losses as olosses, modulations as omod, util as outil
from tests.helpers import lfo_units64 as L
from tests.helpers import lfo_units_cases as C

f32, f64 = np.float32, np.float64


def _rel(a, b):
    return float(np.abs(np.asarray(a, f64) - b).max() / max(float(np.abs(b).max()), 1e-300))


# ==== synthesis ================================================================================================================
@pytest.mark.parametrize("sr", C.SRS)
@pytest.mark.parametrize("shape", L.SHAPES)
def test_phase_argument_and_shapes_vs_oracle(shape, sr):
    n = 882
    for freq, phase in zip(C.RATES, (-6.0, 0.9, 2 * math.pi, 0.0)):
        arg = L.lfo_arg32(np.arange(n), 0, freq, phase, shape, sr)
        f, ph = (freq / 2.0, phase / 2.0) if shape in ("rect_cos", "inv_rect_cos") else (freq, phase)
        assert np.array_equal(arg, omod.lfo_argument(n, sr, f, ph))
        for exp in C.EXPS:
            want = omod.make_mod_signal(n, sr, freq, phase, shape, exp).numpy()
            got, margin = L.lfo_value64(arg, shape, exp)
            if shape in ("tri", "saw", "rsaw"):
                if exp in (1.0, 2.0, 3.0):
                    assert np.array_equal(L.lfo_bits32(arg, shape, exp), want), (shape, exp)     # torch.pow's fast paths
                if exp == 1.0:
                    assert np.array_equal(got, want.astype(f64))
            ok = margin >= C.MARGIN_SYNTH
            tol = 2.0 ** -22 if exp != 0.5 else 2.0 ** -11          # the oracle's own fp32: sqrt near 0 amplifies one rounding of v
            assert float(np.abs(got - want)[ok].max()) <= tol, (shape, exp)


@pytest.mark.parametrize("shape", L.SHAPES)
def test_shape_functions_in_fp64_vs_torch_float64(shape):
    """The same formulas written with torch in float64 from the same fp32 argument (modulations.py:32-54)."""
    arg = L.lfo_arg32(np.arange(2000), 44099, 2.7, 0.9, shape, 441.0)
    a = torch.from_numpy(arg)
    saw = torch.from_numpy(omod.lfo_saw(arg)).double()
    want = {"cos": (torch.cos((a + math.pi).double()) + 1.0) / 2.0, "rect_cos": torch.abs(torch.cos((a + (math.pi / 2.0)).double())),
            "inv_rect_cos": -torch.abs(torch.cos(a.double())) + 1.0, "sqr": (torch.sign(torch.cos((a + math.pi).double())) + 1.0) / 2.0,
            "saw": saw, "rsaw": (1.0 - saw.float()).double(), "tri": torch.where(2 * saw > 1, (2.0 - (2 * saw).float()).double(), 2 * saw)}[shape]
    for exp in C.EXPS:
        got = L.lfo_value64(arg, shape, exp)[0]
        w = want if exp == 1.0 else want ** float(f32(exp))
        assert _rel(got, w.numpy()) <= 1e-12, (shape, exp)


@pytest.mark.parametrize("start", [1, 44099])
def test_start_is_a_crop_of_the_longer_signal(start):
    n = 257
    for shape in L.SHAPES:
        long = omod.make_mod_signal(n + start, 441.0, 2.7, 0.9, shape).numpy()
        got = C.oracle_signal(n, 441.0, 2.7, 0.9, L.SHAPES.index(shape), 1.0, start)
        if shape in ("tri", "saw", "rsaw", "sqr"):
            assert np.array_equal(got, long[start:]), shape
        else:                                                      # torch's vectorised cos: the last bit depends on the position in the row
            assert float(np.abs(got - long[start:]).max()) <= 2.0 ** -22, shape
        f, ph = (2.7 / 2.0, 0.9 / 2.0) if shape in ("rect_cos", "inv_rect_cos") else (2.7, 0.9)
        assert np.array_equal(L.lfo_arg32(np.arange(n), start, 2.7, 0.9, shape, 441.0), omod.lfo_argument(n + start, 441.0, f, ph)[start:])


def test_synth_cases_cover_what_the_gpu_file_claims_and_respect_the_cap():
    cases = C.synth_cases()
    seen, exact = set(), set()
    for case in cases:
        ref, margin, _ = C.synth_ref(case)
        assert np.isfinite(ref).all()
        assert float((margin < C.MARGIN_SYNTH).mean()) <= C.CAP_SYNTH, case["name"]                 # the 1 % exclusion cap
        for b in range(C.SYNTH_B):
            sh, e, st = C.synth_row_params(case, b)
            seen.add((case["n_src"], case["n_out"] == case["n_src"], case["start"] is None, case["exp"] is None, case["shape"] is None))
            if case["n_out"] == case["n_src"]:
                exact.add((sh, e))
    assert {(sh, e) for sh in (L.TRI, L.SAW, L.RSAW) for e in (1.0, 2.0, 3.0)} <= exact
    assert {s[0] for s in seen} == set(C.N_SRC) and any(s[2] for s in seen) and any(s[3] for s in seen) and any(s[4] for s in seen)
    assert {c["n_out"] for c in cases if c["n_src"] == 256} == {256, 1, 345, 513}
    assert {int(s) for c in cases if c["start"] is not None for s in c["start"]} == set(C.STARTS)
    assert {c["sr"] for c in cases} == set(C.SRS) and {float(f) for c in cases for f in c["freq"]} == {float(f32(r)) for r in C.RATES}


def test_synth_gates_come_from_the_oracle():
    gates = C.synth_gates()
    for e, (worst, gate) in gates.items():
        print(f"[measured] exponent {e:g}: oracle worst |value - ref64| {worst:.3e}, gate {gate:.3e}")
        assert gate == max(4.0 * worst, 2.0 ** -22) and np.isfinite(gate)
        # a wrong reference would widen its own gate: the oracle's fp32 error has a ceiling by reasoning -- values in [0, 1] and
        # at most eight roundings of half an ulp of 1; under the square root a perturbation d of v moves the result by sqrt(d) at most
        ceiling = 8 * 2.0 ** -24 if e != 0.5 else math.sqrt(2 * 2.0 ** -23)
        assert worst <= ceiling, (e, worst)
    assert set(gates) == {float(f32(e)) for e in C.EXPS}


# ==== resampling ===============================================================================================================
@pytest.mark.parametrize("n_in,n_out", C.INTERP_PAIRS + ((1, 1), (882, 1765), (255, 345), (257, 1)))
def test_taps_and_interpolation_vs_oracle(n_in, n_out):
    mine, theirs = L.interp_taps32(n_in, n_out), outil.interp_indices_weights(n_in, n_out)
    for a, b in zip(mine, theirs):
        assert np.array_equal(a, b)
    x = np.random.default_rng(n_in + n_out).uniform(-1, 1, (C.INTERP_ROWS, n_in)).astype(f32)
    want = outil.linear_interpolate_last_dim_np(x, n_out).astype(f64)
    got = L.interp64(x, n_in, n_out)
    i0, i1 = mine[0], mine[1]
    bound = np.spacing(np.maximum(np.abs(x[:, i0]), np.abs(x[:, i1])))      # the oracle's two fp32 roundings
    assert (np.abs(got - want) <= bound).all()
    # transpose: the oracle's taps, accumulated another way
    for name, (j0, j_len) in C.interp_windows(n_in, n_out).items():
        dy = C.interp_dy(n_in, n_out, j0, j_len)
        js = np.arange(j0, j0 + j_len)
        want = np.stack([np.bincount(theirs[0][js], theirs[2][js].astype(f64) * r, n_in) + np.bincount(theirs[1][js], theirs[3][js].astype(f64) * r, n_in)
                         for r in dy.astype(f64)])
        assert _rel(L.interp_bwd64(dy, n_in, n_out, j0), want) <= 1e-12, name
        if (n_in, n_out) in C.INTERP_PAIRS:
            err, gate = C.interp_bwd_gate(n_in, n_out, j0, j_len)
            assert gate == max(4.0 * err, 1e-6) and err <= 2e-6, name     # (a wrong reference would widen its own gate)


def test_interp_windows_are_what_they_are_called():
    for n_in, n_out in C.INTERP_PAIRS:
        wins = C.interp_windows(n_in, n_out)
        assert wins["all"] == (0, n_out)
        i0 = L.interp_taps32(n_in, n_out)[0]
        for name, (j0, j_len) in wins.items():
            assert 0 <= j0 and j_len >= 1 and j0 + j_len <= n_out
        if "inside_one_interval" in wins:
            j0, j_len = wins["inside_one_interval"]
            assert len(set(i0[j0:j0 + j_len])) == 1 and (L.interp_taps32(n_in, n_out)[3][j0:j0 + j_len] > 0).all()
        if "two_and_a_half_intervals" in wins and n_in > 5:
            j0, j_len = wins["two_and_a_half_intervals"]
            assert len(set(i0[j0:j0 + j_len])) in (2, 3, 4)
    assert "inside_one_interval" in C.interp_windows(345, 86410) and "two_and_a_half_intervals" in C.interp_windows(345, 86410)
    assert "inside_one_interval" in C.interp_windows(882, 345) and "two_and_a_half_intervals" in C.interp_windows(882, 345)


# ==== corners ==================================================================================================================
def _all_rows(n):
    rows, names = C.corner_stack(n, 130)
    assert set(names) == set(L.designed_rows(n))
    noise = np.random.default_rng(n).uniform(0, 1, (6, n)).astype(f32)
    smooth = (0.5 + 0.4 * np.sin(np.linspace(0, 9, n))[None] * np.linspace(0.3, 1, 4)[:, None]).astype(f32)
    return np.concatenate([rows, noise, smooth])


@pytest.mark.parametrize("n", C.CORNER_N)
def test_corner_helpers_equal_the_oracle(n):
    m = _all_rows(n)
    top, bot = L.corners_ref(m)
    t_o, b_o = omod.find_corners_np(m)
    assert np.array_equal(top, t_o) and np.array_equal(bot, b_o)
    for mc in C.MAX_N_CORNERS:
        want = omod.stretch_corners(torch.from_numpy(m), mc, 0).numpy()
        assert np.array_equal(L.stretch_ref(m, mc), want, equal_nan=True), mc
    for args in C.VALID_ARGS + ((1, 6, 1, 6, int(0.10 * n)),):
        want = [int(omod.check_mod_sig_np(m[r], top[r], bot[r], *args[:4], min_fraction_between_corners=(args[4] + 0.5) / n)) for r in range(len(m))]
        assert L.valid_ref(m, *args).tolist() == want, args
    for k in (1, 2, 8):
        if k <= n:
            assert np.array_equal(L.smoothen_ref(m, k), omod.smoothen_np(m, k))
    assert _rel(L.smoothen_ref(m, n), m.astype(f64).mean(1, keepdims=True)) <= n * 2.0 ** -24


@pytest.mark.parametrize("n", C.CORNER_N)
def test_designed_rows_have_the_listed_corners(n):
    d = L.designed_rows(n)
    for name, v in d.items():
        row = v["row"]
        assert row.shape == (n,) and np.array_equal(row * 64, np.round(row * 64)) and row.min() == 0, name     # on the grid k / 64
        top, bot = L.corners_ref(row[None])
        assert np.nonzero(top[0] == 1)[0].tolist() == v["tops"] and np.nonzero(bot[0] == 1)[0].tolist() == v["bots"], name
        assert top.sum() == v["n_top"] and bot.sum() == v["n_bot"], name
    assert d["monotone"]["n_top"] == d["monotone"]["n_bot"] == 0
    good = d[C.GOOD_ROW]["row"][None]
    assert L.valid_ref(good, 1, 6, 1, 6, int(0.10 * n))[0] == 1 and L.stretch_gain_finite(good, 16)[0]
    assert all(not np.array_equal(L.stretch_ref(good, mc), good) for mc in C.MAX_N_CORNERS)
    for mc in C.MAX_N_CORNERS:
        if mc < 16 or n >= 40:                                    # exactly max_n_corners (stretched) and one more (copied)
            at, above = d[f"alt{mc}"]["row"][None], d[f"alt{mc + 1}"]["row"][None]
            assert d[f"alt{mc}"]["n_top"] + d[f"alt{mc}"]["n_bot"] == mc and d[f"alt{mc + 1}"]["n_top"] + d[f"alt{mc + 1}"]["n_bot"] == mc + 1
            assert not np.array_equal(L.stretch_ref(at, mc), at) and np.array_equal(L.stretch_ref(above, mc), above)
    assert not L.stretch_gain_finite(d["equal_anchors"]["row"][None], 16)[0]
    if n >= 40:
        for c in range(1, 9):
            for cp in range(1, 9):
                v = L.counted_row(n, c, cp)
                top, bot = L.corners_ref(v["row"][None])
                assert (top.sum(), bot.sum()) == (c, cp)
        for g in (8, 9, 10):
            assert d[f"gap{g}_tops"]["gap"] == g and d[f"gap{g}_two_tops_one_bottom"]["gap"] == g
        assert not L.stretch_gain_finite(d["equal_anchors_end"]["row"][None], 16)[0]
        assert d["scaled3"]["row"].max() > 1 and L.corners_ref(d["scaled3"]["row"][None])[1].max() == 4       # a map value above 1
        assert L.corners_ref(d["scaled3_base"]["row"][None])[1].max() == 1
        for name in ("plateau2_top_and_bottom", "plateau3_top_and_bottom"):
            assert d[name]["tops"] == [] and len(d[name]["bots"]) == 1, name      # the nudge: the bottom plateau is a corner, the top is not


@pytest.mark.parametrize("R", C.CORNER_R)
@pytest.mark.parametrize("n", C.CORNER_N)
def test_corner_stacks_put_a_good_row_at_every_workgroup_edge(n, R):
    rows, names = C.corner_stack(n, R)
    assert rows.shape == (R, n)
    for r in {0, R - 1} | {r for r in range(R) if r % 64 in (0, 63)}:
        assert names[r] == C.GOOD_ROW


def test_validity_rows_cannot_pass_vacuously():
    rows, names = C.corner_stack(90, 130, C.VALID_ROWS, C.VALID_GOOD_ROW)
    d = L.designed_rows(90)
    assert all(L.valid_ref(d[C.VALID_GOOD_ROW]["row"][None], *args)[0] == 1 for args in C.VALID_ARGS)
    assert {d[k]["n_top"] for k in names} >= {0, 1, 2, 6, 7} and {d[k]["n_bot"] for k in names} >= {0, 1, 2, 6, 7}
    assert {d[k]["gap"] for k in names} >= {8, 9, 10}
    assert any(d[k]["n_top"] <= 6 and d[k]["n_bot"] > 6 for k in names) and any(d[k]["n_top"] > 6 and d[k]["n_bot"] <= 6 for k in names)
    for args in C.VALID_ARGS:
        share = float(L.valid_ref(rows, *args).mean())
        assert 0.25 <= share <= 0.75, (args, share)


@pytest.mark.parametrize("n", C.CORNER_N)
def test_stretch_gradient_closed_form_vs_float64_autograd(n):
    d = L.designed_rows(n)
    rows = np.stack([v["row"] for v in d.values()])
    for mc in C.MAX_N_CORNERS:
        m = rows[L.stretch_gain_finite(rows, mc)]
        g = C.stretch_dout(n, len(m))
        x = torch.from_numpy(m).double().requires_grad_(True)
        omod.stretch_corners_torch(x, mc, 0).backward(torch.from_numpy(g).double())
        got, want = L.stretch_bwd64(m, g, mc), x.grad.numpy()
        assert float((np.abs(got - want).max(1) / np.abs(want).max(1)).max()) <= 1e-12, mc
        err, gate = C.stretch_bwd_gate(n, mc)
        print(f"[measured] stretch gradient n={n} max_n_corners={mc}: oracle fp32 autograd {err:.3e}, gate {gate:.3e}")
        assert gate == max(4.0 * err, 1e-6) and err <= 2e-6               # (a wrong reference would widen its own gate)


# ==== loss =====================================================================================================================
def _loss_inputs(B, n):
    yield "grid", 1.0, C.loss_grid_inputs(B, n)
    for amp in C.LOSS_AMPLITUDES:
        yield "generic", amp, C.loss_generic_inputs(B, n, amp)


@pytest.mark.parametrize("n", C.LOSS_N)
@pytest.mark.parametrize("B", C.LOSS_B)
def test_loss_reference_vs_float64_autograd_and_exclusion_cap(B, n):
    names = ("l1", "fdl1", "sdl1", "mse")
    for family, amp, (y_hat, y) in _loss_inputs(B, n):
        for w in C.LOSS_W:
            ref = L.lfo_loss64(y_hat, y, w)
            a = torch.from_numpy(y_hat).double().requires_grad_(True)
            t = torch.from_numpy(y).double()
            terms = [olosses.get_loss_func_by_name(k)(a, t) for k in names]
            total = sum(float(f32(wk)) * tk for wk, tk in zip(w, terms) if wk > 0)           # lightning.py:48-52
            total.backward()
            assert _rel(ref["terms"], np.array([float(v) for v in terms])) <= 1e-12
            assert abs(ref["total"] - float(total)) <= 1e-12 * abs(float(total))
            assert _rel(ref["grad"], a.grad.numpy()) <= 1e-12, (family, w)
            low = ref["margin"] < C.MARGIN_LOSS * amp
            if family == "grid":
                assert (ref["margin"][low] == 0).all()                 # on the grid a small margin is an exact zero: nothing is excluded
                e = y_hat.astype(f64) - y
                assert (e == 0).mean() >= 0.3 and (np.diff(e[:, :max(1, n // 4)], axis=1) == 0).all()
            else:
                assert float(low.mean()) <= C.CAP_LOSS, (B, n, w, amp, float(low.mean()))             # the 2 % exclusion cap

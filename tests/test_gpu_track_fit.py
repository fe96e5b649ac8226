"""GPU: the track fit (K23: csrc/track_fit.hip, ``mx_track_fit``; ``modulations.fit_lfo`` beyond K18's limits and
``file_eval.fit_track`` on long tracks) against the definition in numpy, tests/helpers/lfo_fit64.py.

The criteria are those of tests/test_gpu_lfo_fit.py, whose docstring derives them.  The kernel's (shape, rate, phase) is
re-evaluated by the helper in fp64 and its R / Syy may exceed the helper's own minimum by at most GATE = 1e-6: what one swap
of two near-equal candidates can cost when the device's ``cosf`` differs from the correctly rounded cosine by an ulp,
2 sqrt(resid) 3e-7 / std(t) a candidate.  Nothing in that bound depends on n; it presupposes resid <= 1.1e-2, which is
asserted on the helper's result for every row the gate is applied to (clean or 0.02-noise cos, tri and rect_cos on the long
rows; the saws stay on K18's short rows: a clean rsaw of 4097 points is in a neighbouring minimum at 2.1e-2 in the helper
itself).  The shape equals the helper's on clean rows.  amp, offset and resid are within one fp32 rounding (2^-23) of the
helper's fp64 objective on the template ``lfo_value`` has on the device at the kernel's candidate (``make_mod_signals``).

Shapes: the smallest at which this kernel can go wrong.  4097 points (one more than K18 takes; three row tiles) in rows a
stride of n + 3 apart; 345 points on a grid of 639 rates (more than K18's 512; 80 candidate tiles); 16 and 63 points (one row
tile partly filled; 103 x 32 candidates end in a partly filled candidate tile); T - 1, T, T + 1 and 2 T + 17 points around the
row tile T = ``modulations.TRACK_FIT_ROW_TILE``; B = 1.

FAIL WITHOUT THE FEATURE: test_fit_lfo_beyond_k18 (``fit_lfo`` raised MX_ERR_UNSUPPORTED), test_two_rate_track (the parent
fitted the first 4096 points: 1.100 Hz), test_short_track_keeps_its_launch (no ``rate_div`` argument),
test_score_pair_on_a_long_file (fit_points was 4096), and everything that calls ``mx_track_fit``.

Measured on the MI355X: profiles/r25/README.md."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from tests.helpers import lfo_fit64 as h

pytestmark = pytest.mark.gpu
GATE = 1e-6
EPS = 2.0 ** -23
PREMISE = 1.1e-2                                                              # the resid GATE's derivation presupposes
SR = 172.5


@functools.lru_cache(maxsize=None)
def tile():
    from mod_extraction_amd import modulations as M
    return M.TRACK_FIT_ROW_TILE


def spec(name):
    """(n, sr, window, shape names, fit keywords, rows as (shape, rate, phase, noise)) of a case."""
    T = tile()
    narrow = lambda n: (n, SR, (0.9, 1.5), ("cos", "tri"), {}, (("tri", 1.13, 2.0, 0.0),))
    return {
        "n4097": (4097, SR, (0.5, 2.0), ("cos", "rect_cos", "tri"), {},
                  (("cos", 0.83, 1.0, 0.0), ("tri", 1.37, 4.0, 0.02), ("rect_cos", 1.61, 2.5, 0.0))),
        "n345_k639": (345, SR, (0.25, 80.0), ("cos", "rect_cos", "tri"), {}, (("tri", 3.3, 0.7, 0.02), ("cos", 41.0, 5.0, 0.0))),
        "n16": (16, SR, (11.0, 80.0), ("cos", "rect_cos", "tri"), {"rate_div": 16}, (("cos", 17.0, 1.0, 0.0), ("tri", 23.0, 3.0, 0.0))),
        "n63": (63, 31.5, (0.25, 6.0), ("cos", "rect_cos", "tri"), {}, (("rect_cos", 2.2, 0.3, 0.0), ("cos", 1.4, 2.0, 0.02))),
        "T-1": narrow(T - 1), "T": narrow(T), "T+1": narrow(T + 1), "2T+17": narrow(2 * T + 17),
    }[name]


@functools.lru_cache(maxsize=None)
def case(name):
    """(rows (B, n) fp32, the helper's fit of every row, which rows are clean): seeded; shared and not modified."""
    n, sr, window, names, kw, rows = spec(name)
    rng = np.random.default_rng(2500 + n)
    y = np.stack([h.make_row(n, sr, s, f, p, noise=noise, rng=rng) for s, f, p, noise in rows])
    ref = [h.fit_row(r, sr, window[0], window[1], mask=h.mask_of(names), **kw) for r in y]
    return y, ref, [noise == 0.0 for *_, noise in rows]


def raw_track_fit(dev, y, y_stride, B, n, sr, window, mask=0x3F, rate_div=4, J=32, L=4, pad=3):
    """``mx_track_fit`` on a workspace of exactly the planned size and outputs, each with ``pad`` sentinel entries (rows, for
    the table; 64 bytes, for the workspace) behind what the call owns: (outputs, table, workspace, its planned bytes)."""
    from mod_extraction_amd import _hip
    sizes = (ctypes.c_int64 * 2)()
    _hip.call("mx_track_fit_plan", B, n, sr, window[0], window[1], mask, rate_div, J, L, ctypes.addressof(sizes),
              ctypes.addressof(sizes) + 8)
    assert sizes[0] == h.grid_of(n, sr, window[0], window[1], rate_div)[4] and sizes[1] % 8 == 0
    ws = torch.full((sizes[1] + 64,), 0xA5, device=dev, dtype=torch.uint8)
    assert ws.data_ptr() % 16 == 0
    outs = [torch.full((B + pad,), -777, device=dev, dtype=torch.int32)] + \
           [torch.full((B + pad,), -777.0, device=dev, dtype=torch.float32) for _ in range(5)]
    table = torch.full((B + pad, 7), -777.0, device=dev, dtype=torch.float32)
    _hip.call("mx_track_fit", y.data_ptr(), y_stride, B, n, sr, window[0], window[1], mask, rate_div, J, L,
              *[o.data_ptr() for o in outs], table.data_ptr(), ws.data_ptr(), sizes[1], _hip.stream())
    return outs, table, ws, sizes[1]


def as_fit(outs, table, B):
    from mod_extraction_amd import modulations as M
    return M.LFOFit(*[o[:B] for o in outs], table[:B])


def host(fit):
    return {k: v.cpu().numpy() for k, v in fit._asdict().items() if v is not None}


def check(tag, y, sr, fit, ref, clean, allowed):
    """Every row of ``fit`` (an LFOFit with the table) against the helper's ``ref``; prints each figure, then asserts."""
    from mod_extraction_amd import modulations as M
    n = y.shape[1]
    k = host(fit)
    t_dev = M.make_mod_signals(n, sr, fit.rate_hz, fit.phase, fit.shape).cpu().numpy()
    worst = {"excess": -np.inf, "amp": 0.0, "offset": 0.0, "resid": 0.0}
    for b in range(len(y)):
        premise = ref[b]["resid"]
        excess = h.eval_at(y[b], sr, k["shape"][b], k["rate_hz"][b], k["phase"][b])["resid"] - ref[b]["resid"]
        o = h.objective(y[b], t_dev[b])
        at = {"a": float(o["a"][0]), "b": float(o["b"][0]), "resid": float(o["R"][0] / o["Syy"])}
        d_amp = abs(float(k["amp"][b]) - at["a"]) / abs(at["a"])
        d_off = abs(float(k["offset"][b]) - at["b"]) / abs(at["b"])
        d_res = abs(float(k["resid"][b]) - at["resid"])
        print(f"{tag} row {b}: kernel {h.SHAPES[k['shape'][b]]} {k['rate_hz'][b]:.6f} Hz phase {k['phase'][b]:.6f} resid "
              f"{k['resid'][b]:.3e}; helper {h.SHAPES[ref[b]['shape']]} {ref[b]['rate_hz']:.6f} Hz resid {premise:.3e}; excess "
              f"{excess:.3e} amp {d_amp:.3e} offset {d_off:.3e} resid {d_res:.3e}")
        worst = {"excess": max(worst["excess"], excess), "amp": max(worst["amp"], d_amp), "offset": max(worst["offset"], d_off),
                 "resid": max(worst["resid"], d_res)}
        tol = PREMISE
        assert premise <= tol, (b, premise)                                   # the gate below applies to this row
        tol = GATE
        assert excess <= tol, (b, excess)
        if clean[b]:
            assert k["shape"][b] == ref[b]["shape"], b
        tol = EPS
        assert d_amp <= tol, (b, d_amp)
        assert d_off <= tol, (b, d_off)
        assert d_res <= tol, (b, d_res)
        assert 0.0 <= k["phase"][b] < 2.0 * math.pi and k["amp"][b] >= 0.0
        table = k["per_shape_resid"][b]
        assert int(np.argmin(table)) == k["shape"][b] and table[k["shape"][b]] == k["resid"][b]
        assert [bool(np.isfinite(v)) for v in table] == [s in allowed for s in range(7)]
    print(f"{tag}: worst excess {worst['excess']:.3e}, amp {worst['amp']:.3e}, offset {worst['offset']:.3e}, "
          f"resid {worst['resid']:.3e}")


@pytest.mark.parametrize("name", ["n4097", "n345_k639", "n16", "n63", "T-1", "T", "T+1", "2T+17"])
def test_kernel_against_the_helper(dev, name):
    """The new entry point itself, so that the short rows reach it too; rows a stride of n + 3 apart, read in place."""
    n, sr, window, names, kw, _ = spec(name)
    y, ref, clean = case(name)
    B = len(y)
    wide = torch.full((B, n + 3), float("nan"), device=dev)
    wide[:, :n] = torch.from_numpy(y).to(dev)
    outs, table, ws, ws_bytes = raw_track_fit(dev, wide, n + 3, B, n, sr, window, mask=h.mask_of(names), **kw)
    check(name, y, sr, as_fit(outs, table, B), ref, clean, [h.SHAPE_IDS[s] for s in names])
    for o in outs + [table]:
        assert bool((o[B:] == -777).all())
    assert bool((ws[ws_bytes:] == 0xA5).all())                                # nothing behind the reported size is touched


def test_fit_lfo_beyond_k18(dev, monkeypatch):
    """FAILS WITHOUT THE FEATURE.  ``fit_lfo`` on (2, 4097) rows: within the gates, by ``mx_track_fit*`` alone; and on (7, 345)
    default rows it makes only today's ``mx_lfo_fit`` call."""
    from mod_extraction_amd import _hip, modulations as M
    from tests.test_gpu_lfo_fit import case as k18_case
    calls = []
    real = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: calls.append((name, a)) or real(name, *a))
    n, sr, window, names, _, _ = spec("n4097")
    y, ref, clean = case("n4097")
    fit = M.fit_lfo(torch.from_numpy(y[:2]).to(dev), sr, window, shapes=names, per_shape=True)
    assert [c[0] for c in calls] == ["mx_track_fit_plan", "mx_track_fit"]
    check("fit_lfo (2, 4097)", y[:2], sr, fit, ref[:2], clean[:2], [h.SHAPE_IDS[s] for s in names])
    y7, _ = k18_case(345, 0.0)
    yd = torch.from_numpy(y7).to(dev)
    calls.clear()
    short = M.fit_lfo(yd, 172.5)
    assert [c[0] for c in calls] == ["mx_lfo_fit"] and len(calls[0][1]) == 19
    assert calls[0][1][:11] == (yd.data_ptr(), 345, 7, 345, 172.5, 0.25, 8.0, 0x3F, 4, 32, 4)
    assert calls[0][1][11:17] == tuple(o.data_ptr() for o in short[:6]) and calls[0][1][17] is None


@pytest.mark.parametrize("n", [63, 345])
def test_agreement_with_k18(dev, n):
    """K18's own clean rows (tests/test_gpu_lfo_fit.py: six shapes and a second triangle): the new entry point meets the same
    gates; whether (rate, phase) are ``mx_lfo_fit``'s bits is printed, not asserted (K18's coarse stage deals a candidate's
    points to several lanes on a small grid, so its sums are ordered differently)."""
    from mod_extraction_amd import modulations as M
    from tests.test_gpu_lfo_fit import SIZES, case as k18_case
    sr, window = SIZES[n]
    y, ref = k18_case(n, 0.0)
    yd = torch.from_numpy(y).to(dev)
    outs, table, _, _ = raw_track_fit(dev, yd, n, len(y), n, sr, window)
    fit = as_fit(outs, table, len(y))
    check(f"K18 rows n {n}", y, sr, fit, ref, [True] * len(y), range(6))
    k18 = M.fit_lfo(yd, sr, window, per_shape=True)
    same = [bool(torch.equal(a, b)) for a, b in zip(fit, k18)]
    print(f"K18 rows n {n}: bit for bit against mx_lfo_fit (shape, rate, phase, amp, offset, resid, table): {same}")
    assert torch.equal(fit.shape, k18.shape)


def test_plumbing(dev):
    from mod_extraction_amd import modulations as M
    n, sr, window, names, _, _ = spec("n345_k639")
    y, _, _ = case("n345_k639")
    yd = torch.from_numpy(y).to(dev)
    kw = dict(shapes=names, per_shape=True)
    assert M.fit_plan(n, sr, window)[0] == "track_fit"
    compact = M.fit_lfo(yd, sr, window, **kw)
    again = M.fit_lfo(yd, sr, window, **kw)
    assert all(torch.equal(a, b) for a, b in zip(compact, again))            # two launches: the same bits
    wide = torch.full((4, n), float("nan"), device=dev)                       # every other row of a buffer, read in place
    wide[::2] = yd
    view = wide[::2]
    assert view.stride() == (2 * n, 1) and not view.is_contiguous()
    assert all(torch.equal(a, b) for a, b in zip(compact, M.fit_lfo(view, sr, window, **kw)))
    one = M.fit_lfo(yd[1], sr, window, **kw)                                  # B = 1: a 1-d row
    assert all(o.shape[0] == 1 and torch.equal(o[0], c[1]) for o, c in zip(one, compact))
    # a one-shape mask: the answer of that shape in the full table
    tri = M.fit_lfo(yd, sr, window, shapes=["tri"], per_shape=True)
    assert tri.shape.tolist() == [3, 3] and torch.equal(tri.per_shape_resid[:, 3], compact.per_shape_resid[:, 3])
    assert bool(torch.isinf(tri.per_shape_resid[:, [0, 1, 2, 4, 5, 6]]).all()) and torch.equal(tri.resid, tri.per_shape_resid[:, 3])
    # a constant row beside an ordinary one: K18's rule
    y2 = np.stack([np.full(n, 0.3, dtype=np.float32), y[0]])
    k = host(M.fit_lfo(torch.from_numpy(y2).to(dev), sr, window, shapes=["saw", "tri"], per_shape=True))
    assert k["shape"][0] == 3 and k["rate_hz"][0] == np.float32(0.25) and k["phase"][0] == 0.0 and k["amp"][0] == 0.0
    assert k["offset"][0] == np.float32(0.3) and k["resid"][0] == 0.0
    assert [float(v) for v in k["per_shape_resid"][0]] == [np.inf, np.inf, np.inf, 0.0, 0.0, np.inf, np.inf]
    assert k["shape"][1] == 3 and k["per_shape_resid"][1][3] == compact.per_shape_resid[0, 3].item()


def two_rate_track():
    """12 288 points at 172.5 Hz: a 1.1 Hz triangle on the first 4096, a 1.4 Hz triangle on the other 8192, noise 0.02."""
    rng = np.random.default_rng(25)
    return np.concatenate([h.make_row(4096, SR, "tri", 1.1, 0.5, noise=0.02, rng=rng),
                           h.make_row(8192, SR, "tri", 1.4, 0.5, noise=0.02, rng=rng)])


def test_two_rate_track(dev):
    """FAILS WITHOUT THE FEATURE: the parent fitted the first 4096 points and returned 1.100 Hz.  The helper on the whole row
    gives 1.400 Hz with resid 0.56 (the first third does not fit), so the excess gate does not apply here."""
    from mod_extraction_amd.file_eval import fit_track
    from mod_extraction_amd.modulations import SHAPE_IDS
    fit, used = fit_track(torch.from_numpy(two_rate_track()).to(dev), SR, (1.0, 1.5))
    print(f"two-rate track: {used} points, {fit.shape_names()} {float(fit.rate_hz[0]):.5f} Hz resid {float(fit.resid[0]):.4f}")
    assert used == 12288 and int(fit.shape[0]) == SHAPE_IDS["tri"]
    assert abs(float(fit.rate_hz[0]) - 1.4) <= 0.01


def test_short_track_keeps_its_launch(dev, monkeypatch):
    """A 1035-point track is the parent's single ``mx_lfo_fit`` launch at rate_div 4; an explicit ``rate_div`` is honoured on
    whichever route takes it."""
    from mod_extraction_amd import _hip
    from mod_extraction_amd.file_eval import fit_track
    calls = []
    real = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: calls.append((name, a)) or real(name, *a))
    track = torch.from_numpy(h.make_row(1035, SR, "tri", 0.4, 1.0)).to(dev)
    fit, used = fit_track(track, SR)
    assert used == 1035 and [c[0] for c in calls] == ["mx_lfo_fit"]
    assert calls[0][1][:11] == (track.data_ptr(), 1035, 1, 1035, SR, 0.25, 8.0, 0x3F, 4, 32, 4) and len(calls[0][1]) == 19
    calls.clear()
    fit2, used2 = fit_track(track, SR, rate_div=2)
    assert used2 == 1035 and [c[0] for c in calls] == ["mx_lfo_fit"] and calls[0][1][8] == 2
    calls.clear()
    fit8, used8 = fit_track(track, SR, rate_div=16)                           # K = 745: the new route, on the whole track
    assert used8 == 1035 and [c[0] for c in calls] == ["mx_track_fit_plan", "mx_track_fit"] and calls[1][1][8] == 16
    assert fit.shape_names() == fit2.shape_names() == fit8.shape_names() == ["tri"]
    assert max(abs(float(f.rate_hz[0]) - 0.4) for f in (fit, fit2, fit8)) <= 0.01


def test_score_pair_on_a_long_file(dev):
    """FAILS WITHOUT THE FEATURE (fit_points was 4096).  tests/test_gpu_file_eval.py's recording at 25 s: n_t = 4312 track
    points, its stub extractor (the true LFO of every window) and its slow triangle; the rate error is at most twice that of the
    same fit on the TRUE track, the existing file test's rule."""
    from mod_extraction_amd import lightning
    from mod_extraction_amd.file_eval import fit_track, score_pair
    from mod_extraction_amd.modulations import SHAPE_IDS
    from tests.helpers import lfo_stitch64 as S
    from tests.test_gpu_file_eval import N, N_F, RATE, SR as FILE_SR, Stub, spec_of, truth
    L = 25 * FILE_SR
    r = np.random.default_rng(32)
    dry = torch.from_numpy((0.3 * r.standard_normal(L)).astype(np.float32)).to(dev)
    fxp = {"feedback": 0.3, "min_delay_width": 0.5, "width": 0.8, "depth": 0.8, "mix": 0.7}
    mk = lambda **kw: lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=FILE_SR, effect="flanger",
                                                           audio_loss_dict={"esr": 1.0}, **kw).to(dev)
    lfo_full = torch.from_numpy(truth(np.arange(L)).astype(np.float32)).to(dev)
    wet = mk().render(dry.view(1, 1, L), lfo_full.view(1, L), fxp).reshape(L)
    out = score_pair(mk(learned_fx=spec_of(fxp), match_gain="ls"), Stub(wet), dry, wet, n_samples=N)
    n_t = out["track"].numel()
    assert n_t == round(L * N_F / N) == 4312 and out["fit_points"] == n_t and out["n_windows"] == 24
    point_rate = FILE_SR * (n_t - 1) / (L - 1)
    true_track = torch.from_numpy(truth(S.positions(L, n_t)).astype(np.float32)).to(dev)
    fit_true, used = fit_track(true_track, point_rate)
    rate, rate_true = float(out["rate_hz"]), float(fit_true.rate_hz[0])
    print(f"score_pair on 25 s: {n_t} points fitted, rate {rate:.6f} Hz, on the TRUE track {rate_true:.6f} Hz (truth {RATE}), "
          f"resid {float(out['resid']):.3e}, esr {float(out['esr']):.3e}")
    assert used == n_t and int(out["shape"]) == SHAPE_IDS["tri"] == int(fit_true.shape[0])
    assert abs(rate - RATE) <= 2.0 * abs(rate_true - RATE)

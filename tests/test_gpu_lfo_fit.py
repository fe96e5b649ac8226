"""GPU: the LFO fit kernel (csrc/lfo_fit.hip, ``modulations.fit_lfo``) against its definition in numpy
(tests/helpers/lfo_fit64.py), ``synth_from_fit``, the plumbing of the launch, and ``LFOExtraction(fit_metrics=...)``.

The criterion for the search is robust to ties: the kernel's (shape, rate, phase) is re-evaluated by the helper in fp64 and
its R / Syy may exceed the helper's own minimum by at most GATE.  The helper's templates have the correctly rounded fp32
cosine, the device's ``cosf`` may differ from it by an ulp, so near-equal candidates can swap.  amp, offset and resid are
held to one fp32 rounding of the helper's fp64 objective on the template ``lfo_value`` has on the device at the kernel's
candidate (``mx_lfo_synth`` writes it: the contract is about the fp32 values of ``lfo_value``, and offset = mean(y) - a mean(t)
cancels, so an ulp of the cosine in a few points shows in it several times over: 2.9e-7 relative was measured against the
helper's own cosine).

GATE.  Measured on the MI355X (profiles/r18/README.md): the excess is exactly 0 on all 49 rows below (43 in the seven cases, 6 in the mask test) -- the kernel picks the
helper's candidate on every one -- and 4 x 0 is no gate that survives another ``cosf``.  So the gate is what one swap can cost:
two candidates swap only where their R differ by less than what the cosine's difference moves R.  |dt_i| <= 2.5 x 2^-23 (the
device's cosine within 2 ulp of the true one, the helper's within half an ulp, values <= 1), so sqrt(R) moves by at most
a sqrt(n) 3e-7 and R / Syy by 2 sqrt(resid) 3e-7 / std(t); with resid <= 1.1e-2 on these rows and std(t) >= 0.28 for every
shape that is 2.3e-7 a candidate, 4.6e-7 for the pair: GATE = 1e-6.  It is 10 x tighter than the 1e-5 the gate may never exceed
and 1900 x below the smallest runner-up gap tests/test_lfo_fit64.py guarantees on clean rows (1.9e-3 at 16 points), so it cannot
hide a wrong shape.
"""
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests.helpers import lfo_fit64 as h

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = 1e-6
EPS = 2.0 ** -23
# (n, sr, rate window): 2 s rows; 63 and 345 are no multiple of the 32 / 64 lanes a candidate's points are dealt to
SIZES = {16: (8.0, (0.25, 2.0)), 63: (31.5, (0.25, 6.0)), 345: (172.5, (0.25, 8.0)), 4096: (172.5, (0.5, 0.6))}
NAMES7 = h.SHAPES[:6] + ("tri",)


@functools.lru_cache(maxsize=None)
def case(n, noise):
    """(rows (B, n) fp32, the helper's fit of every row): B = 7 (one row at n = 4096), seeded; shared and not modified."""
    sr, (f_lo, f_hi) = SIZES[n]
    rng = np.random.default_rng(1000 * n + int(noise * 1000))
    T = n / sr
    ys = []
    for name in (NAMES7 if n != 4096 else ("tri",)):
        f = float(np.clip(rng.uniform(1.5, 12.0) / T, f_lo * 1.05, f_hi * 0.95)) if n != 4096 else 0.55
        ys.append(h.make_row(n, sr, name, f, rng.uniform(0.0, 2.0 * np.pi), noise=noise, rng=rng))
    y = np.stack(ys)
    return y, [h.fit_row(r, sr, f_lo, f_hi) for r in y]


def host(fit):
    return {k: v.cpu().numpy() for k, v in fit._asdict().items() if v is not None}


def fit_on(dev, y, n, **kw):
    from mod_extraction_amd import modulations as M
    sr, window = SIZES[n]
    return M.fit_lfo(torch.from_numpy(np.ascontiguousarray(y)).to(dev), sr, window, **kw)


@pytest.mark.parametrize("n,noise", [(16, 0.0), (16, 0.02), (63, 0.0), (63, 0.02), (345, 0.0), (345, 0.02), (4096, 0.0)])
def test_kernel_against_the_helper(dev, n, noise):
    sr, _ = SIZES[n]
    from mod_extraction_amd import modulations as M
    y, ref = case(n, noise)
    fit = fit_on(dev, y, n, per_shape=True)
    k = host(fit)
    # the fp32 template of lfo_value at the kernel's candidate, as the device evaluates it (mx_lfo_synth: the same lfo_value)
    t_dev = M.make_mod_signals(n, sr, fit.rate_hz, fit.phase, fit.shape).cpu().numpy()
    worst = {"excess": -np.inf, "amp": 0.0, "offset": 0.0, "resid": 0.0}
    for b in range(len(y)):                                                   # every row, every comparison
        # the search: the helper's own evaluation (its cosine) of the kernel's candidate against the helper's minimum
        excess = h.eval_at(y[b], sr, k["shape"][b], k["rate_hz"][b], k["phase"][b])["resid"] - ref[b]["resid"]
        # amp, offset, resid: the helper's fp64 objective on the template values lfo_value has on the device
        o = h.objective(y[b], t_dev[b])
        at = {"a": float(o["a"][0]), "b": float(o["b"][0]), "resid": float(o["R"][0] / o["Syy"])}
        d_amp = abs(float(k["amp"][b]) - at["a"]) / abs(at["a"])
        d_off = abs(float(k["offset"][b]) - at["b"]) / abs(at["b"])
        d_res = abs(float(k["resid"][b]) - at["resid"])
        print(f"n {n} noise {noise} row {b} {NAMES7[b] if n != 4096 else 'tri'}: kernel {h.SHAPES[k['shape'][b]]} "
              f"{k['rate_hz'][b]:.6f} Hz phase {k['phase'][b]:.6f} resid {k['resid'][b]:.3e}; helper {h.SHAPES[ref[b]['shape']]} "
              f"{ref[b]['rate_hz']:.6f} Hz; excess {excess:.3e} amp {d_amp:.3e} offset {d_off:.3e} resid {d_res:.3e}")
        worst = {"excess": max(worst["excess"], excess), "amp": max(worst["amp"], d_amp), "offset": max(worst["offset"], d_off),
                 "resid": max(worst["resid"], d_res)}
        tol = GATE
        assert excess <= tol, (b, excess)
        if noise == 0.0:
            assert k["shape"][b] == ref[b]["shape"], b
        tol = EPS
        assert d_amp <= tol, (b, d_amp)
        assert d_off <= tol, (b, d_off)
        assert d_res <= tol, (b, d_res)
        assert 0.0 <= k["phase"][b] < 2.0 * math.pi and k["amp"][b] >= 0.0
        assert int(np.argmin(k["per_shape_resid"][b])) == k["shape"][b] and np.isinf(k["per_shape_resid"][b, 6])
        assert k["per_shape_resid"][b, k["shape"][b]] == k["resid"][b]
    print(f"n {n} noise {noise}: worst excess {worst['excess']:.3e}, amp {worst['amp']:.3e}, offset {worst['offset']:.3e}, "
          f"resid {worst['resid']:.3e}")


def synth_rounding(n, fit_row_host, Syy, resid):
    """What the fp32 roundings of ``offset + amp * template`` can add to R / Syy: every point moves by at most
    e = 2^-22 (|offset| + |amp|) (tests/test_lfo_fit64.py), so sqrt(R) moves by at most sqrt(n) e and R / Syy by
    (2 sqrt(R) sqrt(n) e + n e^2) / Syy."""
    e = 2.0 ** -22 * (abs(fit_row_host[0]) + abs(fit_row_host[1]))
    return (2.0 * math.sqrt(resid * Syy) * math.sqrt(n) * e + n * e * e) / Syy


@pytest.mark.parametrize("n,noise", [(63, 0.0), (345, 0.02)])
def test_resynthesis_and_continuation(dev, n, noise):
    from mod_extraction_amd import modulations as M
    sr, _ = SIZES[n]
    y, _ = case(n, noise)
    fit = fit_on(dev, y, n)
    k = host(fit)
    again = M.synth_from_fit(fit, n, sr).cpu().numpy()
    ahead = M.synth_from_fit(fit, n, sr, start=n).cpu().numpy()
    assert again.shape == ahead.shape == y.shape and again.dtype == np.float32
    for b in range(len(y)):
        _, yc, Syy = h.row_stats(y[b])
        d = y[b].astype(np.float64) - again[b].astype(np.float64)
        got = float((d * d).sum() / Syy)
        tol = GATE + synth_rounding(n, (k["offset"][b], k["amp"][b]), Syy, float(k["resid"][b]))
        print(f"n {n} row {b}: resynthesis R / Syy {got:.6e}, kernel resid {k['resid'][b]:.6e}, tol {tol:.2e}")
        assert abs(got - float(k["resid"][b])) <= tol, b
        # the continuation against the helper's: the device cosine within 2 ulp of the true one, the helper's within half
        # an ulp, both of values <= 1 (2.5 x 2^-23 on the template), and the four roundings of the affine map
        row = {key: k[key][b] for key in ("shape", "rate_hz", "phase", "amp", "offset")}
        want = h.synth(row, n, sr, start=n)
        tol = 2.0 ** -21 * (abs(float(row["amp"])) + abs(float(row["offset"])))
        assert float(np.abs(ahead[b] - want).max()) <= tol, b
        if row["shape"] >= 3:                                                 # no cosine in tri / saw / rsaw: the very bits
            assert np.array_equal(again[b], h.synth(row, n, sr)) and np.array_equal(ahead[b], want), b


def raw_fit(dev, y, y_stride, B, n, sr, window, mask=0x3F, rate_div=4, J=32, L=4, pad=3):
    """``mx_lfo_fit`` on output buffers with ``pad`` sentinel entries (rows, for the table) behind the B the kernel owns."""
    from mod_extraction_amd import _hip
    outs = [torch.full((B + pad,), -777, device=dev, dtype=torch.int32)] + \
           [torch.full((B + pad,), -777.0, device=dev, dtype=torch.float32) for _ in range(5)]
    table = torch.full((B + pad, 7), -777.0, device=dev, dtype=torch.float32)
    _hip.call("mx_lfo_fit", y.data_ptr(), y_stride, B, n, sr, window[0], window[1], mask, rate_div, J, L,
              *[o.data_ptr() for o in outs], table.data_ptr(), _hip.stream())
    return outs, table


def test_plumbing(dev):
    from mod_extraction_amd import modulations as M
    n = 63
    sr, window = SIZES[n]
    y, _ = case(n, 0.02)
    yd = torch.from_numpy(y).to(dev)
    compact = M.fit_lfo(yd, sr, window, per_shape=True)
    again = M.fit_lfo(yd, sr, window, per_shape=True)
    assert all(torch.equal(a, b) for a, b in zip(compact, again))            # two launches: the same bits
    # every other row of a (14, n) buffer, read in place
    wide = torch.full((14, n), float("nan"), device=dev)
    wide[::2] = yd
    view = wide[::2]
    assert view.stride() == (2 * n, 1) and not view.is_contiguous()
    strided = M.fit_lfo(view, sr, window, per_shape=True)
    assert all(torch.equal(a, b) for a, b in zip(compact, strided))
    # a sentinel behind every output is untouched, and the direct call writes what fit_lfo returns
    outs, table = raw_fit(dev, wide, 2 * n, 7, n, sr, window)
    for o, c in zip(outs + [table], compact):
        assert torch.equal(o[:7], c) and bool((o[7:] == -777).all())
    # B = 1: a 1-d row, and a single row of the batch
    one = M.fit_lfo(yd[3], sr, window, per_shape=True)
    assert all(o.shape[0] == 1 and torch.equal(o[0], c[3]) for o, c in zip(one, compact))
    assert compact.shape_names() == [h.SHAPES[i] for i in compact.shape.tolist()]


def test_special_rows_known_rate_and_mask(dev):
    from mod_extraction_amd import modulations as M
    from tests.test_lfo_fit64 import anti_row
    n, sr = 48, 24.0
    # a constant row beside an ordinary one
    y = np.stack([np.full(n, 0.3, dtype=np.float32), h.make_row(n, sr, "tri", 1.7, 2.5)])
    k = host(M.fit_lfo(torch.from_numpy(y).to(dev), sr, (0.25, 4.0), shapes=["saw", "tri"], per_shape=True))
    assert k["shape"][0] == 3 and k["rate_hz"][0] == np.float32(0.25) and k["phase"][0] == 0.0 and k["amp"][0] == 0.0
    assert k["offset"][0] == np.float32(0.3) and k["resid"][0] == 0.0
    assert [float(v) for v in k["per_shape_resid"][0]] == [np.inf, np.inf, np.inf, 0.0, 0.0, np.inf, np.inf]
    assert k["shape"][1] == 3 and k["resid"][1] <= 1e-3 and np.isinf(k["per_shape_resid"][1][[0, 1, 2, 5, 6]]).all()
    # no candidate correlates positively: amp 0, resid 1
    ya, kw = anti_row()
    k = host(M.fit_lfo(torch.from_numpy(ya).to(dev), kw["sr"], (kw["f_min"], kw["f_max"]), shapes=["sqr"], n_phases=kw["J"],
                       n_rounds=kw["L"]))
    assert k["shape"][0] == 6 and k["rate_hz"][0] == 2.0 and k["amp"][0] == 0.0 and k["resid"][0] == 1.0 and k["offset"][0] == 0.0
    # K == 1: phase and shape at a known rate
    y = np.stack([h.make_row(n, sr, name, 1.7, 2.5) for name in h.SHAPES[:6]])
    k = host(M.fit_lfo(torch.from_numpy(y).to(dev), sr, (1.7, 1.7)))
    assert k["shape"].tolist() == [0, 1, 2, 3, 4, 5] and (k["rate_hz"] == np.float32(1.7)).all() and (k["resid"] <= 1e-3).all()
    # a mask restricts the answer
    k = host(M.fit_lfo(torch.from_numpy(y).to(dev), sr, (0.25, 4.0), shapes=["cos", "saw"], per_shape=True))
    assert set(k["shape"].tolist()) <= {0, 4} and k["shape"][0] == 0 and k["shape"][4] == 4
    assert np.isinf(k["per_shape_resid"][:, [1, 2, 3, 5, 6]]).all() and np.isfinite(k["per_shape_resid"][:, [0, 4]]).all()
    for b in range(6):
        want = h.fit_row(y[b], sr, 0.25, 4.0, mask=h.mask_of(["cos", "saw"]))
        at = h.eval_at(y[b], sr, k["shape"][b], k["rate_hz"][b], k["phase"][b])
        tol = GATE
        assert at["resid"] - want["resid"] <= tol, b


class Stub(torch.nn.Module):
    """A model that returns the LFO it was built with."""

    def __init__(self, lfo):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.lfo = lfo

    def forward(self, x):
        return self.lfo.unsqueeze(1), None


def step_case(dev, factor=1.0):
    """8 labels of 345 points (cos, tri and the rectified cosines at 0.8 .. 3 Hz: the shapes whose objective is smooth in the
    rate), a stub that returns the label synthesised at ``factor`` times its rate, and the batch."""
    from mod_extraction_amd import modulations as M
    g = torch.Generator().manual_seed(7)
    freq = (0.8 + 2.2 * torch.rand(8, generator=g)).to(dev)
    phase = (2.0 * math.pi * torch.rand(8, generator=g)).to(dev)
    shape = torch.tensor([0, 1, 2, 3, 0, 1, 2, 3], dtype=torch.int32, device=dev)
    label = M.make_mod_signals(345, 172.5, freq, phase, shape)
    hat = label if factor == 1.0 else M.make_mod_signals(345, 172.5, freq * factor, phase, shape)
    audio = torch.zeros(8, 1, 88200, device=dev)
    return Stub(hat), (audio, audio.clone(), label, None), freq


def test_step_logs_the_fit_metrics(dev, monkeypatch):
    from mod_extraction_amd import _hip, lightning, modulations as M
    names = []
    real = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: names.append(name) or real(name, *a))
    kw = dict(sr=44100, model_smooth_n_frames=1, loss_dict={"l1": 1.0, "mse": 0.0})
    model, batch, _ = step_case(dev)
    plain = lightning.LFOExtraction(model, **kw).to(dev)
    names.clear()                                                             # the label's own synthesis
    _, data, _ = plain.validation_step(batch)
    assert "mx_lfo_fit" not in names and len(names) > 0 and "lfo_fit" not in data
    assert sorted(plain.logged) == ["val/l1", "val/loss", "val/mse"]
    parent_names = list(names)
    step = lightning.LFOExtraction(model, fit_metrics={"rate_hz": [0.25, 8.0]}, **kw).to(dev)
    names.clear()
    step.training_step(batch)
    assert "mx_lfo_fit" not in names and sorted(step.logged) == ["train/l1", "train/loss", "train/mse"]
    names.clear()
    step.logged.clear()
    _, data, _ = step.validation_step(batch)
    assert names == parent_names + ["mx_lfo_fit"]                             # one launch on the 2 B rows, nothing else
    log = {key: float(v[0]) for key, v in step.logged.items()}
    assert sorted(log) == sorted(["val/l1", "val/loss", "val/mse"] + [f"val/{m}" for m in step.FIT_METRIC_NAMES])
    assert all(v[0].is_cuda and v[0].ndim == 0 for v in step.logged.values())
    assert log["val/fit_rate_err_hz"] == 0.0 and log["val/fit_rate_err_rel"] == 0.0 and log["val/fit_shape_acc"] == 1.0
    assert log["val/fit_resid"] == log["val/fit_label_resid"] and log["val/fit_resid"] <= 1e-3
    fit = data["lfo_fit"]
    assert isinstance(fit, M.LFOFit) and fit.shape.shape == (8,) and fit.shape.tolist() == [0, 1, 2, 3, 0, 1, 2, 3]


def test_step_reports_a_rate_that_is_a_quarter_off(dev):
    """The stub returns the label at 1.25 x its rate.  Each fit is within the last round's spacing d = df / 2^L of its row's
    true rate (tests/test_lfo_fit64.py), so |rate_hat - rate| / rate is within (1.25 d + d) / (f - d) of 0.25."""
    from mod_extraction_amd import lightning
    model, batch, freq = step_case(dev, 1.25)
    step = lightning.LFOExtraction(model, sr=44100, model_smooth_n_frames=1, fit_metrics={"rate_hz": [0.25, 8.0]}).to(dev)
    _, data, _ = step.validation_step(batch)
    d = 172.5 / (4 * 345) / 2 ** 4
    tol = 2.25 * d / (float(freq.min()) - d)
    rel = float(step.logged["val/fit_rate_err_rel"][0])
    print(f"fit_rate_err_rel {rel:.5f} (tol {tol:.5f} around 0.25), shape acc {float(step.logged['val/fit_shape_acc'][0])}")
    assert abs(rel - 0.25) <= tol
    assert float(step.logged["val/fit_shape_acc"][0]) == 1.0
    assert abs(float(step.logged["val/fit_rate_err_hz"][0]) - 0.25 * float(freq.mean())) <= 2.25 * d


def test_validate_runs_on_the_fit_config(dev):
    """scripts/validate.py's path on configs/eval_lfo_fit.yml (freshly initialised weights, one validation batch)."""
    from mod_extraction_amd import cli
    cwd = os.getcwd()
    os.chdir(os.path.join(ROOT, "scripts"))
    try:
        c = cli.CustomLightningCLI(args=["validate", "-c", "../configs/eval_lfo_fit.yml"], run=False, device=dev,
                                   allow_missing_ckpt=True, trainer_defaults={"log_fn": None, "limit_val_batches": 1})
    finally:
        os.chdir(cwd)
    c.prepare_data_stream()
    c.model.eval()
    metrics = c.trainer.validate(c.model, c.datamodule)
    fit_keys = {f"val/{m}" for m in c.model.FIT_METRIC_NAMES}
    assert set(metrics) == {"val/l1", "val/fdl1", "val/sdl1", "val/mse", "val/loss"} | fit_keys and len(fit_keys) == 5
    assert all(math.isfinite(float(v)) for v in metrics.values())
    assert 0.0 <= metrics["val/fit_shape_acc"] <= 1.0 and 0.0 <= metrics["val/fit_resid"] <= 1.0
    assert 0.0 <= metrics["val/fit_label_resid"] <= 1.0 and metrics["val/fit_rate_err_hz"] <= 7.75

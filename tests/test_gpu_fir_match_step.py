"""GPU: lightning.LFOExtractionThroughEffect(match_fir=...) -- the per-clip FIR match (mod_extraction_amd/fir_match.py, K21)
inside the effect-rendered step, at B = 6, N = 22 272 as tests/test_gpu_gain_step.py.  Flanger rows from the batcher.

1. the node by hand: with match_fir=5 the node's wet_hat, loss and d loss / d LFO are torch.equal to render with stash,
   match_fir, effect_loss_grad, match_fir_backward, _adjoint_rows.
2. no argument, no change: without match_fir a training step's _hip.call names are those of a default-constructed step (no
   mx_fir_match_*), loss, wet_hat and dmod are torch.equal and the logged keys the same; with it the six launches are added,
   once each and in order, and nothing else.
3. tone at the label: wet := the batch's wet through [0.2, 0.6, 0.15] in fp64 on the host, rounded once; {"esr": 1}, the LFO
   at the label.  The re-render is the batch's wet bit for bit, so five centred taps hold the filter exactly up to the
   O(K / N) bias of the zero-extended fit.  Requirement: esr(match_fir=5) < 1e-3 esr(match_gain="ls") (an fp64 stand-in
   measured 2.5e-9 times).  FAILS WITHOUT THE FEATURE.
4. fractional lag at the label: wet := 0.5 x the wet delayed by 0.4 samples (129-tap Hann-windowed sinc, fp64, host).
   Requirement: esr(match_fir=9) < 0.2 esr(match_gain="ls") (the stand-in measured 0.066 times; the margin of 3 is because
   the stand-in is not the project's flanger).  FAILS WITHOUT THE FEATURE.
5. chain gradient against fp64: d loss / d LFO under "mse" against tests/helpers/flanger_adjoint64_lr.py chained through
   tests/helpers/fir_match64.py: 3e-6 norm-wise over the batch, the gate of the K20 step test.
6. fit: the 60-step recipe of tests/test_gpu_gain_step.py on the tone-filtered wet with and without match_fir; the fitted
   values are printed, and only "the final loss with it is below the one without" is asserted.
7. mixed batch: five kinds, finite everywhere, zero gradient on dry rows, data_dict["fir"] of shape (B, K) in training and
   in validation, the three fir/ metrics logged as device scalars.
The two ratios and the fitted values are on record in profiles/r22/fir_match.md."""
import math

import numpy as np
import pytest
import torch

from tests.helpers import fir_match64 as fm
from tests.helpers.flanger_adjoint64_lr import flanger_adjoint64_lr
from tests.test_gpu_flanger_grad import normwise
from tests.test_gpu_gain_step import off_label
from tests.test_gpu_mixed_step import batch_of, cnn

pytestmark = pytest.mark.gpu
SR = 44100
B, N = 6, 22272
FIVE = ("flanger", "chorus", "phaser", "tremolo", "dry")
TONE = (0.2, 0.6, 0.15)
FIR_CALLS = ["mx_fir_match_partials", "mx_fir_match_solve", "mx_fir_match_apply", "mx_fir_match_bwd_partials",
             "mx_fir_match_bwd_solve", "mx_fir_match_bwd_apply"]


def tone_filtered(wet):
    """wet[n] -> 0.2 wet[n] + 0.6 wet[n - 1] + 0.15 wet[n - 2] in fp64 on the host, rounded once."""
    w = wet[:, 0].cpu().numpy().astype(np.float64)
    out = np.stack([np.convolve(r, TONE)[:w.shape[1]] for r in w])
    return torch.as_tensor(out.astype(np.float32)).unsqueeze(1).to(wet.device)


def half_level_delayed(wet, lag=0.4):
    """0.5 x wet delayed by ``lag`` samples: a 129-tap Hann-windowed sinc in fp64 on the host, rounded once."""
    w = wet[:, 0].cpu().numpy().astype(np.float64)
    t = np.arange(-64, 65)
    g = np.sinc(t - lag) * np.hanning(129)
    out = np.stack([0.5 * np.convolve(r, g)[64:64 + w.shape[1]] for r in w])
    return torch.as_tensor(out.astype(np.float32)).unsqueeze(1).to(wet.device)


def esr_at_the_label(dry, wet, mod, fxp, **kw):
    from mod_extraction_amd import lightning
    step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect="flanger", audio_loss_dict={"esr": 1}, **kw)
    with torch.no_grad():
        loss, _ = step.audio_loss(mod, dry, wet, fxp)
    return float(loss), step


def test_the_node_by_hand(dev):
    from mod_extraction_amd import lightning
    from mod_extraction_amd.effect_losses import effect_loss_grad, effect_loss_terms
    from mod_extraction_amd.fir_match import match_fir, match_fir_backward
    weights = {"mrstft": 1.0, "l1": 0.5}
    dry, wet, mod, fxp = batch_of(dev, ("flanger",), B, N, 61)
    wet = tone_filtered(wet)
    step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect="flanger", audio_loss_dict=weights,
                                                match_fir=5)
    h0 = off_label(mod, dev)
    h = h0.clone().requires_grad_(True)
    loss, wet_hat = step.audio_loss(h, dry, wet, fxp)
    loss.backward()
    taps_of_node = step._fir.taps.clone()
    dry_r, wet_r = dry[:, 0], wet[:, 0]
    consts = step.clip_constants(fxp, B, dev)
    rendered, stashes = step._render_rows(dry_r, h0, consts, stash=True)
    m = match_fir(rendered, wet_r, 5, 2, 1e-6, 1e-8, 20.0)
    values = {}
    dz = effect_loss_grad(m.z.unsqueeze(1), wet, weights, values=values, **step._grad_modules())
    dy = match_fir_backward(dz, rendered, wet_r, m, 1e-6, 1e-8, 2)
    dmod = step._adjoint_rows(dy, dry_r, h0, consts, stashes)
    terms = {"mrstft": values["mrstft"] / 1.0}
    terms["l1"] = effect_loss_terms(m.z.unsqueeze(1), wet)["l1"]
    want = step.weighted_sum(terms, step.audio_loss_dict)
    assert int(m.flags.sum()) == 0 and not torch.equal(m.z, rendered) and dy.data_ptr() != dz.data_ptr()
    assert torch.equal(wet_hat, m.z.unsqueeze(1)) and torch.equal(taps_of_node, m.taps)
    assert torch.equal(loss.detach(), want) and torch.equal(h.grad, dmod)
    assert float(h.grad.abs().max()) > 0
    with torch.no_grad():                                                       # the no-grad branch matches too; render() does not
        loss_v, hat_v = step.audio_loss(h0, dry, wet, fxp)
    assert torch.equal(hat_v, wet_hat) and math.isfinite(float(loss_v))
    assert torch.equal(step.render(dry, h0, fxp), rendered.unsqueeze(1))


def test_no_argument_no_change(dev, monkeypatch):
    from mod_extraction_amd import _hip, lightning
    dry, wet, mod, fxp = batch_of(dev, FIVE, B, N, 62)
    names = []
    real = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (names.append(name), real(name, *a))[1])

    def run(**kw):
        torch.manual_seed(3)
        step = lightning.LFOExtractionThroughEffect(cnn(N), sr=SR, effect=FIVE, audio_loss_dict={"mrstft": 1.0, "l1": 0.5},
                                                    **kw).to(dev).train()
        keys = []
        keep = step.log
        step.log = lambda n, v: (keys.append(n), keep(n, v))[1]
        del names[:]
        step.training_step((dry, wet, mod, fxp)).backward()
        called = list(names)
        h = off_label(mod, dev).requires_grad_(True)
        loss, wet_hat = step.audio_loss(h, dry, wet, fxp)
        loss.backward()
        return step, called, set(keys), loss.detach(), wet_hat, h.grad

    default, calls_d, keys_d, loss_d, hat_d, grad_d = run()
    off, calls_o, keys_o, loss_o, hat_o, grad_o = run(match_fir=None, match_fir_centre=3, match_fir_ridge=1e-3, match_fir_eps=1e-6,
                                                      match_fir_max_gain=5.0)
    on, calls_on, keys_on, _, _, _ = run(match_fir=9)
    assert calls_o == calls_d and not any(n.startswith("mx_fir_") for n in calls_o)
    assert torch.equal(loss_o, loss_d) and torch.equal(hat_o, hat_d) and torch.equal(grad_o, grad_d)
    assert keys_o == keys_d and off.step_metric_names == default.step_metric_names == []
    assert list(off.state_dict()) == list(default.state_dict()) == list(on.state_dict())
    assert [n for n in calls_on if n.startswith("mx_fir_")] == FIR_CALLS
    assert [n for n in calls_on if not n.startswith("mx_fir_")] == calls_d
    assert keys_on == keys_d | {"fir/dc_gain", "fir/l1", "fir/flagged"}


def test_tone_at_the_label(dev):
    dry, wet, mod, fxp = batch_of(dev, ("flanger",), B, N, 63)
    target = tone_filtered(wet)
    with_fir, step = esr_at_the_label(dry, target, mod, fxp, match_fir=5)
    with_gain, _ = esr_at_the_label(dry, target, mod, fxp, match_gain="ls")
    plain, _ = esr_at_the_label(dry, target, mod, fxp)
    print(f"tone: esr match_fir=5 {with_fir:.3e}, match_gain=ls {with_gain:.3e}, neither {plain:.3e}; ratio fir / ls "
          f"{with_fir / with_gain:.3e}; taps of row 0 {step._fir.taps[0].tolist()}")
    assert int(step._fir.flags.sum()) == 0
    assert with_fir < 1e-3 * with_gain


def test_fractional_lag_at_the_label(dev):
    dry, wet, mod, fxp = batch_of(dev, ("flanger",), B, N, 64)
    target = half_level_delayed(wet)
    with_fir, step = esr_at_the_label(dry, target, mod, fxp, match_fir=9)
    with_gain, _ = esr_at_the_label(dry, target, mod, fxp, match_gain="ls")
    plain, _ = esr_at_the_label(dry, target, mod, fxp)
    print(f"lag 0.4: esr match_fir=9 {with_fir:.3e}, match_gain=ls {with_gain:.3e}, neither {plain:.3e}; ratio fir / ls "
          f"{with_fir / with_gain:.3e}; taps of row 0 {step._fir.taps[0].tolist()}")
    assert int(step._fir.flags.sum()) == 0
    assert with_fir < 0.2 * with_gain


def test_chain_gradient_against_fp64(dev):
    from mod_extraction_amd import lightning
    K, c, ridge, eps = 9, 4, 1e-6, 1e-8
    dry, wet, mod, fxp = batch_of(dev, ("flanger",), B, N, 65)
    wet = tone_filtered(wet)
    step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect="flanger", audio_loss_dict={"mse": 1.0},
                                                match_fir=K)
    h0 = off_label(mod, dev)
    h = h0.clone().requires_grad_(True)
    loss, wet_hat = step.audio_loss(h, dry, wet, fxp)
    loss.backward()
    assert float(fxp["feedback"].max()) <= 0.7
    consts = {k: v.cpu().numpy() for k, v in step.clip_constants(fxp, B, dev).items()}
    x, y = dry[:, 0].cpu().numpy(), wet[:, 0].cpu().numpy()
    M = step.max_delay_samples
    fwd = flanger_adjoint64_lr(x, h0.cpu().numpy(), consts, M, np.zeros((B, N)))["fwd"]["y32"]
    ref = fm.rows64(fwd, y, K, c, ridge, eps, 20.0)
    assert np.array_equal(step._fir.taps.cpu().numpy(), ref["taps"]) and ref["flag"].sum() == 0
    z32 = wet_hat[:, 0].cpu().numpy()
    assert (np.abs(z32 - ref["z64"]) <= 2.0 ** -23 * ref["scale"]).all()
    dz = 2.0 * (z32.astype(np.float64) - y) / (B * N)                           # d mse / d z, 'mean' over the batch
    back = fm.rows_backward64(dz, fwd, y, ref, c, ridge, eps)
    want = flanger_adjoint64_lr(x, h0.cpu().numpy(), consts, M, back["dy_hat"])["dmod"]
    err = normwise(h.grad.cpu().numpy(), want, slice(None))
    print(f"chain gradient: norm-wise error of d loss / d LFO {err:.3e} (gate 3e-6), max |dmod| {np.abs(want).max():.3e}")
    assert err < 3e-6


def fit_fir(dev, match_fir):
    """The recipe of tests/test_gpu_gain_step.py::fit_gain on the tone-filtered wet."""
    from mod_extraction_amd import data_modules, lightning
    one = lambda v: (v, v)
    truth = {"feedback": 0.25, "min_delay_width": 1.0, "width": 1.0, "depth": 1.0, "mix": 1.0}
    spec = {"feedback": {"min": 0.0, "max": 0.95, "init": 0.5}, "depth": {"min": 0.0, "max": 1.0, "init": 0.6},
            "mix": {"min": 0.0, "max": 1.0, "init": 0.6}, "width": 1.0, "min_delay_width": 1.0}
    torch.manual_seed(31)
    np.random.seed(31)
    batcher = data_modules.SyntheticFxBatcher(B, N, SR, ("flanger",), dev, audio_seed=31, fixed_lead=0,
                                              flanger_fx=dict({k: one(v) for k, v in truth.items()}, max_min_delay_ms=1.0,
                                                              max_lfo_delay_ms=4.0))
    dry, wet, mod, fxp = batcher.render(batcher.sample_params())
    wet = tone_filtered(wet)
    step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect="flanger", max_lfo_delay_ms=4.0,
                                                learned_fx={"flanger": spec}, match_fir=match_fir).to(dev)
    lf = step.learned_fx
    opt = torch.optim.Adam([lf.raw], lr=0.05)
    start = lf.values().detach().cpu().numpy()
    first = None
    for _ in range(60):
        opt.zero_grad()
        loss, _ = step.audio_loss(mod, dry, wet, {})
        loss.backward()
        opt.step()
        first = loss.detach() if first is None else first
    with torch.no_grad():
        final = float(step.audio_loss(mod, dry, wet, {})[0])
    end = lf.values().detach().cpu().numpy()
    values = dict(zip(lf.names, end.tolist()))
    return lf.names, start, end, float(first), final, values


def test_fit_on_the_tone_filtered_wet(dev):
    names, start, end, first, final, v = fit_fir(dev, 5)
    _, start0, end0, first0, final0, v0 = fit_fir(dev, None)
    print(f"match_fir=5: loss {first:.6e} -> {final:.6e}; without: loss {first0:.6e} -> {final0:.6e}")
    for i, full in enumerate(names):
        print(f"  {full}: {start[i]:.4f} -> {end[i]:.4f} with match_fir; {start0[i]:.4f} -> {end0[i]:.4f} without")
    dm = lambda d: d["flanger.depth"] * d["flanger.mix"]
    print(f"  feedback (truth 0.25): {v['flanger.feedback']:.4f} with, {v0['flanger.feedback']:.4f} without; depth * mix (truth 1): "
          f"{dm(v):.4f} with, {dm(v0):.4f} without")
    assert final < final0


def test_mixed_batch(dev):
    from mod_extraction_amd import lightning
    Bm, K = 10, 9
    dry, wet, mod, fxp = batch_of(dev, FIVE, Bm, N, 66)
    wet = (0.5 * wet).contiguous()
    torch.manual_seed(2)
    step = lightning.LFOExtractionThroughEffect(cnn(N), sr=SR, effect=FIVE, audio_loss_dict={"mrstft": 1.0, "esr": 0.5},
                                                match_fir=K).to(dev).train()
    seen = []
    keep = step.log
    step.log = lambda n, v: (seen.append((n, v)), keep(n, v))[1]
    h = off_label(mod, dev).requires_grad_(True)
    loss, wet_hat = step.audio_loss(h, dry, wet, fxp)
    loss.backward()
    dry_rows = [i for i in range(Bm) if FIVE[i % len(FIVE)] == "dry"]
    assert math.isfinite(float(loss.detach())) and torch.isfinite(wet_hat).all() and torch.isfinite(h.grad).all()
    assert dry_rows == [4, 9] and bool((h.grad[dry_rows] == 0).all()) and float(h.grad.abs().max()) > 0
    assert step._fir.taps.shape == (Bm, K) and torch.isfinite(step._fir.taps).all()
    # a dry row at half level: h = 0.5 at the centre is exact, so the ridge-regularised fit leaves at most
    # lambda |h|^2 = 1e-6 R[0] / 4 of residual energy against |y|^2 = R[0] / 4: an esr of 1e-6 (plus roundings ~1e-14)
    resid = (wet_hat[dry_rows, 0].double() - wet[dry_rows, 0].double()).pow(2).sum(1) / wet[dry_rows, 0].double().pow(2).sum(1)
    assert float(resid.max()) < 2e-6 and float((step._fir.taps[dry_rows, 4] - 0.5).abs().max()) < 0.05
    loss, data, _ = step.common_step((dry, wet, mod, fxp), is_training=True)
    loss.backward()
    assert data["fir"].shape == (Bm, K) and data["fir"].is_cuda and math.isfinite(float(loss)) and "gain" not in data
    assert all(p.grad is None or torch.isfinite(p.grad).all() for p in step.parameters())
    logged = dict(seen)
    for k in ("fir/dc_gain", "fir/l1", "fir/flagged"):
        assert logged[k].is_cuda and logged[k].ndim == 0 and math.isfinite(float(logged[k])), k
    assert float(logged["fir/flagged"]) == float((step._fir.flags != 0).float().mean())
    del seen[:]
    _, data_v, _ = step.validation_step((dry, wet, mod, fxp))
    assert data_v["fir"].shape == (Bm, K) and not any(n.startswith("fir/") for n, _ in seen)
    assert torch.isfinite(data_v["wet_hat"]).all()

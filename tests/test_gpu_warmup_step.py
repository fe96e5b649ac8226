"""GPU: lightning.LFOExtractionThroughEffect(warmup_ms=...) -- the loss warm-up window for chunks cut from the inside of a
recording, at B = 4, N = 22 272 (the step tests' geometry).  Flanger at 1 + 10 ms: a delay line of M = 485 samples.

The "recording" of tests 1, 2 and 4: 3 N noise samples a row at 0.3, a full-rate LFO, rendered by the project's flanger in
ONE full-rate launch; the chunk starts at s = 20 M, a multiple of M, so a re-render of the chunk writes sample n into the slot
the recording wrote sample s + n into.  On [s, s + N) the recording's LFO is the kernel's own upsampling (``mod_up``) of a
low-rate label, outside it the same sine continues.

1. exactly zero (FAILS WITHOUT THE FEATURE): feedback 0, the label, {mse, l1, esr}, warmup_ms = 11 (P = 485 = M): every term
   is exactly 0 -- slots, ring contents and LFO bits coincide from sample M on -- in the training node and under no_grad.
   Without warmup_ms the esr is above 1e-3 (fp64: 1.2e-2).
2. feedback 0.5, P = 4851 >= 10 M: the windowed esr against the same quantity from tests/helpers/flanger_adjoint64.forward
   on the same rows (gate: twice the helper's value plus 1e-9); and below 1 / 20 of the step's esr without the window, the
   ratio also at most twice the helper's ratio (plus 1e-7: the 1e-9 above over an esr of 1e-2).  The fp64 ratio is printed.
3. the node by hand: with warmup_ms the node's loss, wet_hat and d loss / d LFO are torch.equal to its launch sequence written
   out here (views, the match on the window, the zeroed head of dy, the adjoints) for match_fir=5, match_gain="ls" and no
   match; the taps are those of fir_match.match_fir on the two views.
4. d loss / d LFO under mse against tests/helpers/flanger_adjoint64_lr fed a dy that is zero on [:P]: 3e-6 norm-wise, the gate
   of the gain and FIR step tests for this chain.
5. a phaser batch with the data path's random leads, at the label: mrstft with a 50 ms warm-up is strictly below the value
   without; both are printed, no ratio is asserted.
6. warmup_ms=None (and 0) makes exactly the parent's _hip.call sequence, with equal loss, wet_hat and gradient and the same
   logged keys and data_dict keys; with warmup_ms the same launches run (no new entry point).
7. a mixed batch of all five kinds trains and validates with a window: finite, zero gradient on dry rows, wet_hat (B, 1, N)
   with the un-matched render on [:P], data_dict["warmup"] = P."""
import math

import numpy as np
import pytest
import torch

from tests.helpers import flanger_adjoint64 as fa
from tests.helpers.flanger_adjoint64_lr import flanger_adjoint64_lr
from tests.test_gpu_flanger_grad import normwise
from tests.test_gpu_gain_step import off_label
from tests.test_gpu_mixed_step import batch_of, cnn

pytestmark = pytest.mark.gpu
SR = 44100
B, N = 4, 22272
M = 485
START = 20 * M
FIVE = ("flanger", "chorus", "phaser", "tremolo", "dry")
_CACHE = {}


def mk(**kw):
    from mod_extraction_amd import lightning
    return lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect="flanger", **kw)


def recording(dev, feedback):
    """(dry chunk, wet chunk (B, 1, N), label (B, n_mod), fx_params, the recording's dry and full-rate LFO (B, 3 N), consts)
    of the module docstring, built once per feedback and never written afterwards."""
    if feedback in _CACHE:
        return _CACHE[feedback]
    from mod_extraction_amd import fx
    r = np.random.default_rng(23)
    L, n_mod = 3 * N, N // 100
    file_dry = torch.from_numpy((0.3 * r.standard_normal((B, L))).astype(np.float32)).to(dev)
    rate = np.asarray([1.3, 0.7, 2.1, 3.4])[:, None]
    phase = 2 * np.pi * r.random((B, 1))
    lfo = lambda t: 0.5 + 0.45 * np.sin(2 * np.pi * rate * t / SR + phase)          # t in samples of the recording
    label = torch.from_numpy(lfo(START + np.arange(n_mod) * (N - 1) / (n_mod - 1)).astype(np.float32)).to(dev)
    fxp = {"feedback": torch.full((B,), float(feedback), device=dev),
           "min_delay_width": torch.from_numpy(r.random(B).astype(np.float32)).to(dev),
           "width": torch.from_numpy((0.5 + 0.5 * r.random(B)).astype(np.float32)).to(dev),
           "depth": torch.from_numpy((0.5 + 0.5 * r.random(B)).astype(np.float32)).to(dev),
           "mix": torch.from_numpy((0.5 + 0.5 * r.random(B)).astype(np.float32)).to(dev)}
    step = mk()
    assert step.max_delay_samples == M
    consts = step.clip_constants(fxp, B, dev)
    geo = step._mixed_rows(B, dev)
    dry = file_dry[:, START:START + N].contiguous()
    mod_up = torch.empty((B, N), device=dev, dtype=torch.float32)
    fx.flanger_forward(dry, label, consts, geo["max_delay"], geo["max_delay_max"], mod_up=mod_up)   # the kernel's own upsampling
    file_lfo = torch.from_numpy(lfo(np.arange(L)[None, :]).astype(np.float32)).to(dev)
    assert float((file_lfo[:, START:START + N] - mod_up).abs().max()) < 1e-3       # the continuation is smooth at both ends
    file_lfo[:, START:START + N] = mod_up
    file_wet = fx.flanger_forward(file_dry, file_lfo, consts, geo["max_delay"], geo["max_delay_max"])   # ONE full-rate launch
    wet = file_wet[:, START:START + N].contiguous()
    out = (dry.unsqueeze(1), wet.unsqueeze(1), label, fxp, file_dry, file_lfo, consts)
    _CACHE[feedback] = out
    return out


def esr64(y_hat, y, P, eps=1e-8):
    d = (y_hat[:, P:] - y[:, P:]) ** 2
    return float(np.mean(d.sum(1) / ((y[:, P:] ** 2).sum(1) + eps)))


def test_exactly_zero_at_the_label(dev):
    dry, wet, label, fxp, *_ = recording(dev, 0.0)
    weights = {"mse": 1.0, "l1": 1.0, "esr": 1.0}
    step = mk(audio_loss_dict=weights, warmup_ms=11.0)
    P = step.warmup_samples
    assert P == M and START % M == 0
    terms = {}
    keep = step.log
    step.log = lambda n, v: (terms.__setitem__(n, float(v)), keep(n, v))[1]
    h = label.clone().requires_grad_(True)
    loss, wet_hat = step.audio_loss(h, dry, wet, fxp, prefix="train")
    loss.backward()
    head = float((wet_hat[..., :P] - wet[..., :P]).abs().max())
    print(f"with warmup_ms = 11 (P = {P}): terms {terms}, loss {float(loss.detach())!r}; max |wet_hat - wet| on [:P] {head:.3e}")
    assert torch.equal(wet_hat[..., P:], wet[..., P:]) and head > 1e-3
    assert terms == {"train/mse": 0.0, "train/l1": 0.0, "train/esr": 0.0} and float(loss.detach()) == 0.0
    assert bool((h.grad == 0).all())
    with torch.no_grad():
        loss_v, hat_v = step.audio_loss(label, dry, wet, fxp)
    assert float(loss_v) == 0.0 and torch.equal(hat_v, wet_hat)
    plain = mk(audio_loss_dict=weights)
    with torch.no_grad():
        loss_p, _ = plain.audio_loss(label, dry, wet, fxp, prefix="val")
    esr = float(plain.logged["val/esr"][-1])
    print(f"without warmup_ms: esr {esr:.3e}, loss {float(loss_p):.3e} (fp64 figure for this geometry: 1.2e-2)")
    assert esr > 1e-3


def test_feedback_against_fp64(dev):
    dry, wet, label, fxp, file_dry, file_lfo, consts = recording(dev, 0.5)
    step = mk(audio_loss_dict={"esr": 1.0}, warmup_ms=110.0)
    P = step.warmup_samples
    assert P == 4851 and P >= 10 * M
    with torch.no_grad():
        windowed = float(step.audio_loss(label, dry, wet, fxp)[0])
        whole = float(mk(audio_loss_dict={"esr": 1.0}).audio_loss(label, dry, wet, fxp)[0])
    # the same rows in fp64: the recording up to the chunk's end (the effect is causal), and the chunk from an empty line
    c = {k: v.cpu().numpy() for k, v in consts.items()}
    end = START + N
    rec = fa.forward(file_dry[:, :end].cpu().numpy(), file_lfo[:, :end].cpu().numpy(), c, M)["y"][:, START:]
    chunk = fa.forward(dry[:, 0].cpu().numpy(), file_lfo[:, START:end].cpu().numpy(), c, M)["y"]
    windowed64, whole64 = esr64(chunk, rec, P), esr64(chunk, rec, 0)
    print(f"feedback 0.5: esr on [P:], P = {P}: step {windowed:.3e}, fp64 {windowed64:.3e}; esr on the whole clip: step "
          f"{whole:.3e}, fp64 {whole64:.3e}; ratio step {windowed / whole:.3e}, fp64 {windowed64 / whole64:.3e}")
    assert windowed <= 2.0 * windowed64 + 1e-9
    assert windowed < whole / 20.0
    assert windowed / whole <= 2.0 * (windowed64 / whole64) + 1e-7


@pytest.mark.parametrize("match", ["fir", "gain", "none"])
def test_the_node_by_hand(dev, match):
    from mod_extraction_amd.effect_losses import effect_loss_grad, effect_loss_terms
    from mod_extraction_amd.fir_match import match_fir, match_fir_backward
    from mod_extraction_amd.gain import match_gain, match_gain_backward
    weights = {"mrstft": 1.0, "l1": 0.5}
    dry, wet, mod, fxp = batch_of(dev, ("flanger",), B, N, 71)
    wet = (0.5 * wet + 0.2 * wet.roll(1, -1)).contiguous()
    kw = {"fir": {"match_fir": 5}, "gain": {"match_gain": "ls"}, "none": {}}[match]
    step = mk(audio_loss_dict=weights, warmup_ms=50.0, **kw)
    P = step.warmup_samples
    assert P == 2205
    h0 = off_label(mod, dev)
    h = h0.clone().requires_grad_(True)
    loss, wet_hat = step.audio_loss(h, dry, wet, fxp)
    loss.backward()
    taps_of_node = step._fir.taps.clone() if match == "fir" else None
    # the launch sequence, by hand
    dry_r, wet_r = dry[:, 0], wet[:, 0]
    consts = step.clip_constants(fxp, B, dev)
    rendered, stashes = step._render_rows(dry_r, h0, consts, stash=True)
    seen, target = rendered[:, P:], wet_r[:, P:]
    assert seen.stride() == (N, 1) and target.stride() == (N, 1) and seen.data_ptr() == rendered.data_ptr() + 4 * P
    dy = torch.full((B, N), float("nan"), device=dev)
    dy[:, :P] = 0.0
    if match == "fir":
        m = match_fir(seen, target, 5, 2, 1e-6, 1e-8, 20.0)
        z = m.z
    elif match == "gain":
        m = match_gain(seen, target, "ls", 1e-8, (0.05, 20.0))
        z = m.z
    else:
        z = seen
    values = {}
    dz = effect_loss_grad(z.unsqueeze(1), target.unsqueeze(1), weights, values=values, **step._grad_modules())
    assert dz.shape == (B, N - P)
    if match == "fir":
        match_fir_backward(dz, seen, target, m, 1e-6, 1e-8, 2, out=dy[:, P:])
        assert torch.equal(taps_of_node, m.taps) and int(m.flags.sum()) == 0
    elif match == "gain":
        match_gain_backward(dz, seen, target, m, "ls", 1e-8, out=dy[:, P:])
    else:
        dy[:, P:] = dz
    dmod = step._adjoint_rows(dy, dry_r, h0, consts, stashes)
    terms = {"mrstft": values["mrstft"] / 1.0, "l1": effect_loss_terms(z.unsqueeze(1), target.unsqueeze(1))["l1"]}
    want = step.weighted_sum(terms, step.audio_loss_dict)
    assert wet_hat.shape == (B, 1, N)
    assert torch.equal(wet_hat[:, 0, P:], z) and torch.equal(wet_hat[:, 0, :P], rendered[:, :P])
    assert torch.equal(loss.detach(), want) and torch.equal(h.grad, dmod) and float(h.grad.abs().max()) > 0
    if match != "none":
        assert not torch.equal(z, seen)
    with torch.no_grad():                                                       # the no-grad branch matches too; render() does not
        loss_v, hat_v = step.audio_loss(h0, dry, wet, fxp)
    assert torch.equal(hat_v, wet_hat) and abs(float(loss_v) - float(want)) <= 1e-5 * float(want)
    assert torch.equal(step.render(dry, h0, fxp), rendered.unsqueeze(1))
    # and the window changes the answer: the same step without it
    other, _ = mk(audio_loss_dict=weights, **kw).audio_loss(h0.clone().requires_grad_(True), dry, wet, fxp)
    assert not torch.equal(other.detach(), want)


def test_chain_gradient_against_fp64(dev):
    dry, wet, label, fxp, *_ = recording(dev, 0.5)
    step = mk(audio_loss_dict={"mse": 1.0}, warmup_ms=110.0)
    P = step.warmup_samples
    h0 = off_label(label, dev)
    h = h0.clone().requires_grad_(True)
    loss, wet_hat = step.audio_loss(h, dry, wet, fxp)
    loss.backward()
    consts = {k: v.cpu().numpy() for k, v in step.clip_constants(fxp, B, dev).items()}
    x, y = dry[:, 0].cpu().numpy(), wet[:, 0].cpu().numpy()
    z32 = wet_hat[:, 0].cpu().numpy()
    dy = np.zeros((B, N))
    dy[:, P:] = 2.0 * (z32[:, P:].astype(np.float64) - y[:, P:]) / (B * (N - P))     # d mse / d z, 'mean' over the window
    ref = flanger_adjoint64_lr(x, h0.cpu().numpy(), consts, M, dy)
    assert np.array_equal(z32, ref["fwd"]["y32"])
    mse64 = float(((z32[:, P:].astype(np.float64) - y[:, P:]) ** 2).mean())
    assert abs(float(loss.detach()) - mse64) <= 1e-4 * mse64                             # a sanity check of the window's mean, not a gate
    err = normwise(h.grad.cpu().numpy(), ref["dmod"], slice(None))
    inside = int(math.ceil(P * (h0.size(1) - 1) / (N - 1)))                     # LFO frames that lie wholly inside the warm-up
    print(f"chain gradient with dy zero on [:{P}]: norm-wise error {err:.3e} (gate 3e-6), max |dmod| {np.abs(ref['dmod']).max():.3e}; "
          f"max |dmod| on the first {inside - 1} frames {np.abs(ref['dmod'][:, :inside - 1]).max():.3e}")
    assert err < 3e-6


def test_phaser_at_the_label(dev):
    from mod_extraction_amd import lightning
    from tests.test_gpu_phaser_step import batch_of as phaser_batch
    dry, wet, mod, fxp = phaser_batch(dev, B, N, 7, fixed_lead=None)            # the data path's random leads
    assert int(fxp["lead"].max()) > 0
    mkp = lambda **kw: lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect="phaser",
                                                            audio_loss_dict={"mrstft": 1.0}, **kw)
    with torch.no_grad():
        without = float(mkp().audio_loss(mod, dry, wet, fxp)[0])
        windowed = float(mkp(warmup_ms=50.0).audio_loss(mod, dry, wet, fxp)[0])
    print(f"phaser at the label, leads {fxp['lead'].tolist()}: mrstft {without:.6e} without, {windowed:.6e} with warmup_ms = 50")
    assert math.isfinite(windowed) and windowed < without


def test_none_is_the_parents_call_sequence(dev, monkeypatch):
    from mod_extraction_amd import _hip, lightning
    dry, wet, mod, fxp = batch_of(dev, FIVE, 5, N, 72)
    names = []
    real = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (names.append((name, a)), real(name, *a))[1])

    def run(**kw):
        torch.manual_seed(3)
        step = lightning.LFOExtractionThroughEffect(cnn(N), sr=SR, effect=FIVE, audio_loss_dict={"mrstft": 1.0, "l1": 0.5},
                                                    match_fir=5, **kw).to(dev).train()
        keys = []
        keep = step.log
        step.log = lambda n, v: (keys.append(n), keep(n, v))[1]
        del names[:]
        loss, data, _ = step.common_step((dry, wet, mod, fxp), is_training=True)
        loss.backward()
        called = [n for n, _ in names]
        del names[:]
        h = off_label(mod, dev).requires_grad_(True)
        loss, wet_hat = step.audio_loss(h, dry, wet, fxp)
        loss.backward()
        sizes = [(n, [v for v in a if isinstance(v, int) and 0 < v < 1 << 32]) for n, a in names]
        return step, called, sizes, set(keys), set(data), loss.detach(), wet_hat, h.grad

    default, calls_d, sizes_d, keys_d, data_d, loss_d, hat_d, grad_d = run()
    for kw in ({"warmup_ms": None}, {"warmup_ms": 0}, {"warmup_ms": 0.011}):
        off, calls_o, sizes_o, keys_o, data_o, loss_o, hat_o, grad_o = run(**kw)
        assert calls_o == calls_d and sizes_o == sizes_d                       # the same launches with the same sizes and strides
        assert torch.equal(loss_o, loss_d) and torch.equal(hat_o, hat_d) and torch.equal(grad_o, grad_d)
        assert keys_o == keys_d and data_o == data_d and "warmup" not in data_o
        assert list(off.state_dict()) == list(default.state_dict()) and off.step_metric_names == default.step_metric_names
    on, calls_on, sizes_on, keys_on, data_on, loss_on, hat_on, grad_on = run(warmup_ms=50.0)
    assert calls_on == calls_d and keys_on == keys_d and data_on == data_d | {"warmup"}     # no new entry point, no new metric
    assert sizes_on != sizes_d and not torch.equal(loss_on, loss_d)
    assert list(on.state_dict()) == list(default.state_dict())


def test_mixed_batch(dev):
    from mod_extraction_amd import lightning
    Bm, K = 10, 9
    dry, wet, mod, fxp = batch_of(dev, FIVE, Bm, N, 73)
    wet = (0.5 * wet).contiguous()
    torch.manual_seed(2)
    step = lightning.LFOExtractionThroughEffect(cnn(N), sr=SR, effect=FIVE, audio_loss_dict={"mrstft": 1.0, "esr": 0.5},
                                                match_fir=K, warmup_ms=110.0).to(dev).train()
    P = step.warmup_samples
    h = off_label(mod, dev).requires_grad_(True)
    loss, wet_hat = step.audio_loss(h, dry, wet, fxp)
    loss.backward()
    dry_rows = [i for i in range(Bm) if FIVE[i % len(FIVE)] == "dry"]
    assert math.isfinite(float(loss.detach())) and torch.isfinite(wet_hat).all() and torch.isfinite(h.grad).all()
    assert bool((h.grad[dry_rows] == 0).all()) and float(h.grad.abs().max()) > 0
    assert wet_hat.shape == (Bm, 1, N) and torch.equal(wet_hat[dry_rows, 0, :P], dry[dry_rows, 0, :P])   # un-matched on [:P]
    # matched on [P:]: a dry row at half level leaves at most the ridge's 1e-6 of residual energy (tests/test_gpu_fir_match_step.py)
    resid = (wet_hat[dry_rows, 0, P:].double() - wet[dry_rows, 0, P:].double()).pow(2).sum(1) / wet[dry_rows, 0, P:].double().pow(2).sum(1)
    assert float(resid.max()) < 2e-6
    loss, data, _ = step.common_step((dry, wet, mod, fxp), is_training=True)
    loss.backward()
    assert data["warmup"] == P == 4851 and data["wet_hat"].shape == (Bm, 1, N) and data["fir"].shape == (Bm, K)
    assert math.isfinite(float(loss.detach())) and all(p.grad is None or torch.isfinite(p.grad).all() for p in step.parameters())
    _, data_v, _ = step.validation_step((dry, wet, mod, fxp))
    assert data_v["warmup"] == P and torch.isfinite(data_v["wet_hat"]).all()
    assert torch.equal(data_v["wet_hat"][dry_rows, 0, :P], dry[dry_rows, 0, :P])

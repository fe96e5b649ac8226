"""GPU: lightning.LFOExtractionThroughEffect(learned_fx=...) -- the effect's parameters as trainable quantities of the
audio-loss step (fx.LearnedFxParams, csrc/fx_params.hip).

3. consistency with the unlearned step: B = 6, N = 22 272, kinds (flanger, chorus, phaser, tremolo, dry, flanger) on the
   batcher's draw, every (kind, name) pair learned.  The kernel's fp32 values, broadcast by kind into plain (B,) fx_params
   tensors and run through a step WITHOUT learned_fx, give the same wet_hat, loss and d loss / d LFO, torch.equal.
4. end-to-end parameter gradient: B = 5, one row per kind, N = 4096, n_mod = 17, audio_loss_dict {"l1": 1.0}.  The step's
   d loss / d raw against the fp64 adjoint helpers (flanger_adjoint64_lr, tremolo_adjoint64, phaser_adjoint64 at the osc
   row the scan read and the output-clip decisions it took), fed the step's own dy and chained through the helper's map
   (tests/helpers/fx_params64.py).  The chain factor is exact in fp64, so the gates are the ones the project holds these
   parameter gradients to, normalised as their own tests normalise them (max |difference| over the rows of a launch /
   max |reference|): 1e-5 for the flanger / chorus constants and the tremolo's d mix, 1.8e-4 for the phaser's parameters.
5. it fits: the LFO held at the label, constant true parameters, the learned ones start away from the truth; 60 Adam steps on
   raw.  Final loss < first loss and every learned value is closer to its truth than at the start (the recipe of
   test_it_optimises; the ratios are printed, not gated).  Flanger (feedback, depth, mix), phaser (depth, feedback),
   tremolo (mix).
6. real-pair shape: (dry, wet, None, None) batches, the flanger with all five names learned or fixed, Spectral2DCNN, three
   trainer.Trainer steps through a stub data module: finite losses, raw and the extractor's first weight both moved,
   fx/flanger.feedback among the logged metrics; with one needed name missing the step raises a ValueError that names it.
7. every source in one batch: ``clip_constants`` alone (no audio), with ``learned_fx`` and with a zero-weight ``fx_head``, on
   B = 6 rows of (flanger, chorus, phaser, tremolo, dry, flanger) whose constants come from fixed numbers, learned values,
   (B,) batch tensors and python floats at once.  Every vector, on the rows of the families that read it, is torch.equal to
   the value formed in numpy from the rounding rule; the batch's tensors are not written; with every name covered and no
   ``fx_params`` the cached vectors are rewritten in place."""
import math

import numpy as np
import pytest
import torch

from tests.helpers import fx_params64 as h
from tests.helpers import phaser_adjoint64 as pa
from tests.helpers.flanger_adjoint64_lr import flanger_adjoint64_lr
from tests.helpers.tremolo_adjoint64 import tremolo_adjoint64
from tests.test_gpu_mixed_step import batch_of, cnn
from tests.test_gpu_phaser_grad import gpu_decisions, reference

pytestmark = pytest.mark.gpu
SR = 44100
FIVE = ("flanger", "chorus", "phaser", "tremolo", "dry")
UNIT = {"min": 0.0, "max": 1.0, "init": 0.5}
DELAY = {"feedback": {"min": 0.0, "max": 0.7, "init": 0.3}, "min_delay_width": UNIT, "width": UNIT, "depth": UNIT, "mix": UNIT}
ALL = {"flanger": DELAY, "chorus": DELAY, "tremolo": {"mix": UNIT},
       "phaser": {"depth": {"min": 0.2, "max": 1.0, "init": 0.6}, "feedback": {"min": -0.7, "max": 0.7, "init": 0.2},
                  "centre_frequency_hz": {"min": 200.0, "max": 4000.0, "init": 1000.0}, "mix": UNIT}}


def spread_raw(lf, seed, span):
    raw = np.random.default_rng(seed).uniform(-span, span, lf.raw.numel())
    with torch.no_grad():
        lf.raw.copy_(torch.tensor(raw, dtype=torch.float32))


def smooth_lfo(dev, B, n, seed):
    g = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, n)[None, :]
    v = 0.5 + 0.4 * np.sin(2 * np.pi * (g.uniform(1.0, 2.5, (B, 1)) * t + g.uniform(0, 1, (B, 1))))
    return torch.tensor(v, dtype=torch.float32, device=dev)


def test_consistency_with_the_unlearned_step(dev):
    from mod_extraction_amd import fx, lightning
    from mod_extraction_amd.util import linear_interpolate_last_dim
    kinds = FIVE + ("flanger",)
    B, N, n_frames = 6, 22272, 88
    weights = {"mrstft": 1.0, "l1": 0.5}
    dry, wet, mod, _ = batch_of(dev, kinds, B, N, 21, fixed_lead=0)
    learned = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect=kinds, audio_loss_dict=weights,
                                                   learned_fx=ALL).to(dev)
    spread_raw(learned.learned_fx, 5, 2.0)
    plain = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect=kinds, audio_loss_dict=weights)
    t = torch.linspace(0.0, 1.0, n_frames, device=dev)
    bump = 0.1 * torch.sin(2 * math.pi * (1.5 * t[None, :] + torch.arange(B, device=dev)[:, None] / B))
    h0 = (linear_interpolate_last_dim(mod, n_frames, align_corners=True) + bump).clamp(0.0, 1.0)
    ha = h0.clone().requires_grad_(True)
    loss_a, hat_a = learned.audio_loss(ha, dry, wet, None)
    loss_a.backward()
    values = learned._fx_values
    assert values.shape == (15,) and values.dtype == torch.float32
    # the kernel's values, broadcast by kind into plain per-row tensors (0.5 where a kind has no such parameter)
    names = learned.learned_fx.names
    fxp = {}
    for name in ("feedback", "min_delay_width", "width", "depth", "mix", "centre_frequency_hz"):
        rows = [values[names.index(f"{k}.{name}")] if f"{k}.{name}" in names else torch.tensor(0.5, device=dev)
                for k in kinds]
        fxp[name] = torch.stack(rows).contiguous()
    hb = h0.clone().requires_grad_(True)
    loss_b, hat_b = plain.audio_loss(hb, dry, wet, fxp)
    loss_b.backward()
    print(f"consistency: loss {float(loss_a):.6e} / {float(loss_b):.6e}, {int((hat_a != hat_b).sum())} of {hat_a.numel()} "
          f"samples and {int((ha.grad != hb.grad).sum())} of {ha.grad.numel()} gradient values differ")
    assert float(loss_a) > 0 and float(ha.grad.abs().max()) > 0 and not torch.equal(hat_a[:4], dry[:4])
    assert torch.equal(hat_a, hat_b) and torch.equal(loss_a.detach(), loss_b.detach()) and torch.equal(ha.grad, hb.grad)
    assert torch.equal(hat_a[4], dry[4]) and bool((ha.grad[4] == 0).all())              # the dry row
    assert learned.learned_fx.raw.grad is not None and torch.isfinite(learned.learned_fx.raw.grad).all()
    # render() and the no-grad branch use the learned values too
    assert torch.equal(learned.render(dry, h0, None), hat_a)
    with torch.no_grad():
        assert torch.equal(learned.audio_loss(h0, dry, wet, None)[1], hat_a)
    # precedence: a batch that carries fx_params is overridden on the learned rows -- here on all of them
    other = {k: torch.full((B,), 0.123, device=dev) for k in fxp}
    keep = {k: v.clone() for k, v in other.items()}
    assert torch.equal(learned.render(dry, h0, other), hat_a)
    assert all(torch.equal(other[k], keep[k]) for k in other)                           # and the batch's tensors are not written


def test_parameter_gradient_against_fp64(dev):
    from mod_extraction_amd import fx, lightning
    from mod_extraction_amd.effect_losses import effect_loss_grad
    B, N, n_mod = 5, 4096, 17
    g = torch.Generator().manual_seed(44)
    dry = (0.3 * torch.randn(B, 1, N, generator=g)).to(dev)
    wet = (0.3 * torch.randn(B, 1, N, generator=g)).to(dev)
    step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect=FIVE, audio_loss_dict={"l1": 1.0},
                                                learned_fx=fx.LearnedFxParams(ALL, raw_gain=2.0)).to(dev)
    lf = step.learned_fx
    spread_raw(lf, 9, 0.75)
    hl = smooth_lfo(dev, B, n_mod, 10).requires_grad_(True)
    loss, wet_hat = step.audio_loss(hl, dry, wet, None)
    loss.backward()
    got = lf.raw.grad.double().cpu().numpy()
    assert got.shape == (15,) and np.isfinite(got).all()
    consts = {k: v.clone() for k, v in step.clip_constants(None, B, dev).items()}
    dy = effect_loss_grad(wet_hat, wet, {"l1": 1.0}, **step._grad_modules())
    assert dy.shape == (B, N)
    x_np, dy_np, mod_np = dry[:, 0].cpu().numpy(), dy.cpu().numpy(), hl.detach().cpu().numpy()
    m = step._mixed_rows(B, dev)
    ref = {}                                                                            # (slot name, row) -> fp64 gradient
    for r in (0, 1):                                                                    # flanger, chorus
        c = {k: consts[k][r:r + 1].cpu().numpy() for k in fx.PARAM_GRADS + ("one_minus_mix",)}
        out = flanger_adjoint64_lr(x_np[r:r + 1], mod_np[r:r + 1], c, int(m["max_delay"][r]), dy_np[r:r + 1])
        assert np.array_equal(wet_hat[r, 0].cpu().numpy(), out["fwd"]["y32"][0])        # the forward is the fp32 reference
        for k in fx.PARAM_GRADS:
            ref[(k, r)] = float(out[k][0])
    out = tremolo_adjoint64(x_np[3:4], mod_np[3:4], consts["mix"][3:4].cpu().numpy(), dy_np[3:4],
                            omm=consts["one_minus_mix"][3:4].cpu().numpy())
    ref[("mix", 3)] = float(out["dmix"][0])
    pc = {k: consts[k][2:3].contiguous() for k in fx.PHASER_PARAM_GRADS}
    _, st, mod_g = fx.phaser_forward_stash_lr(dry[2:3, 0].contiguous(), pc, None, SR, N, hl.detach()[2:3].contiguous())
    osc = (np.float32(1.0) - np.float32(2.0) * mod_g.cpu().numpy()).astype(np.float32)
    params = {k: v.cpu().numpy() for k, v in pc.items()}
    pref, recompute = reference(x_np[2:3], osc, params, 0, dy_np[2:3], with_recompute=True)
    mine = gpu_decisions(st, N, N)
    flips = int((mine != pref["pass_m"]).sum())
    print(f"phaser row: {flips} output-clip decisions differ between the scan forward and the sequential fp32 forward")
    if flips:
        pref = recompute(mine)
    for k in fx.PHASER_PARAM_GRADS:
        ref[(k, 2)] = float(pref[k][0])
    # chain through the helper's map: d raw[e] = g[slot, row of the kind] * sample count * d value / d raw
    tab_f, tab_i = lf.tab_f.cpu().numpy(), lf.tab_i.cpu().numpy()
    raw = lf.raw.detach().double().cpu().numpy()
    dv = h.dvalue_draw(raw, tab_f[0], tab_f[1], tab_i[0], lf.raw_gain)
    ml, mm = m["max_lfo_delay"].double().cpu().numpy(), m["max_min_delay"].double().cpu().numpy()
    gate = {"flanger": 1e-5, "chorus": 1e-5, "tremolo": 1e-5, "phaser": 1.8e-4}
    per_row = {}                                                                        # entry -> (got, want) as per-clip gradients
    for e, full in enumerate(lf.names):
        kind, name = full.split(".")
        row = FIVE.index(kind)
        slot = h.NAME_SLOT[name]
        count = ml[row] if slot == "lfo_scale" else mm[row] if slot == "min_delay" else 1.0
        per_row[full] = (got[e] / (dv[e] * count), ref[(slot, row)])
        want_raw = ref[(slot, row)] * count * dv[e]
        print(f"{full}: d loss / d raw {got[e]:+.6e}, fp64 {want_raw:+.6e}")
    # the flanger and the chorus row are one launch: a parameter's error is taken over both, as test_gpu_flanger_grad does
    worst = {}
    for name in ("feedback", "min_delay_width", "width", "depth", "mix"):
        a = np.asarray([per_row[f"{k}.{name}"] for k in ("flanger", "chorus")])
        worst[f"delay.{name}"] = float(np.abs(a[:, 0] - a[:, 1]).max() / np.abs(a[:, 1]).max())
    for full in [n for n in lf.names if n.split(".")[0] in ("tremolo", "phaser")]:
        a, b = per_row[full]
        worst[full] = abs(a - b) / abs(b)
    print({k: f"{v:.2e}" for k, v in worst.items()})
    for k, v in worst.items():
        if k.startswith("phaser"):
            assert v <= 1.8e-4, k
        else:
            assert v <= 1e-5, k
    assert gate["phaser"] == 1.8e-4


def fit(dev, effect, truth_fx, spec, truths, names_in_batch):
    """60 Adam steps on raw with the LFO held at the label; returns (first loss, final loss, start values, end values)."""
    from mod_extraction_amd import data_modules, lightning
    B, N = 6, 22272
    torch.manual_seed(31)
    np.random.seed(31)
    batcher = data_modules.SyntheticFxBatcher(B, N, SR, (effect,), dev, audio_seed=31, fixed_lead=0, **truth_fx)
    dry, wet, mod, fxp = batcher.render(batcher.sample_params())
    for k, v in truths.items():
        assert bool((fxp[k] == v).all()), k                                             # constant true parameters
    step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect=effect, max_lfo_delay_ms=4.0,
                                                learned_fx={effect: spec}).to(dev)
    lf = step.learned_fx
    batch_fx = {k: fxp[k] for k in names_in_batch}
    opt = torch.optim.Adam([lf.raw], lr=0.05)
    start = lf.values().detach().cpu().numpy()
    losses = []
    for _ in range(60):
        opt.zero_grad()
        loss, _ = step.audio_loss(mod, dry, wet, batch_fx)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    with torch.no_grad():
        final = float(step.audio_loss(mod, dry, wet, batch_fx)[0])
    first = float(losses[0])
    end = lf.values().detach().cpu().numpy()
    print(f"{effect}: loss {first:.6e} -> {final:.6e}, ratio {final / first:.4f}")
    for i, full in enumerate(lf.names):
        tv = truths[full.split(".")[1]]
        print(f"  {full}: {start[i]:.4f} -> {end[i]:.4f} (truth {tv}), distance ratio {abs(end[i] - tv) / abs(start[i] - tv):.4f}")
    assert final < first
    for i, full in enumerate(lf.names):
        tv = truths[full.split(".")[1]]
        assert abs(end[i] - tv) < abs(start[i] - tv), full


def test_it_fits_flanger(dev):
    one = lambda v: (v, v)
    truth = {"feedback": 0.25, "min_delay_width": 1.0, "width": 1.0, "depth": 1.0, "mix": 1.0}
    fit(dev, "flanger", {"flanger_fx": dict({k: one(v) for k, v in truth.items()}, max_min_delay_ms=1.0, max_lfo_delay_ms=4.0)},
        {"feedback": {"min": 0.0, "max": 0.95, "init": 0.5}, "depth": {"min": 0.0, "max": 1.0, "init": 0.6},
         "mix": {"min": 0.0, "max": 1.0, "init": 0.6}, "width": 1.0, "min_delay_width": 1.0},
        {k: truth[k] for k in ("feedback", "depth", "mix")}, ())


def test_it_fits_phaser(dev):
    truth = {"depth": 0.8, "centre_frequency_hz": 1000.0, "feedback": 0.5, "mix": 1.0}
    fit(dev, "phaser", {"phaser_fx": {k: (v, v) for k, v in truth.items()}},
        {"depth": {"min": 0.0, "max": 1.0, "init": 0.5}, "feedback": {"min": -0.9, "max": 0.9, "init": 0.2}},
        {k: truth[k] for k in ("depth", "feedback")}, ("centre_frequency_hz", "mix"))


def test_it_fits_tremolo(dev):
    fit(dev, "tremolo", {"tremolo_fx": {"mix": (0.7, 0.7)}}, {"mix": {"min": 0.0, "max": 1.0, "init": 0.3}}, {"mix": 0.7}, ())


class PairStub:
    """A data module of recorded pairs in miniature: (dry, wet, None, None) batches, as RandomAudioChunkDryWetDataModule's."""

    def __init__(self, dry, wet):
        self.dry, self.wet, self.batch_size = dry, wet, dry.size(0)

    def train_steps_per_epoch(self):
        return 3

    def val_steps_per_epoch(self):
        return 1

    def train_batch(self):
        return self.dry, self.wet, None, None

    val_batch = train_batch


def test_real_pair_shape(dev):
    from mod_extraction_amd import lightning, optim, trainer
    B, N = 4, 22272
    dry, wet, _, _ = batch_of(dev, ("flanger",), B, N, 41)
    spec = {"flanger": {"feedback": {"min": 0.0, "max": 0.95, "init": 0.3}, "depth": {"min": 0.0, "max": 1.0, "init": 0.5},
                        "mix": {"min": 0.0, "max": 1.0, "init": 0.5}, "width": 1.0, "min_delay_width": 0.5}}
    torch.manual_seed(4)
    step = lightning.LFOExtractionThroughEffect(cnn(N), sr=SR, effect="flanger", learned_fx=spec).to(dev).train()
    opt = optim.FlatAdamW(step.parameters(), lr=1e-4, betas=(0.8, 0.99))
    raw0 = step.learned_fx.raw.detach().clone()
    w0 = next(step.model.parameters()).detach().clone()
    seen = []
    keep = step.log
    step.log = lambda n, v: (seen.append((n, v)), keep(n, v))[1]
    hist = trainer.Trainer(max_epochs=1, log_fn=None).fit(step, PairStub(dry, wet), opt)
    losses = [float(v) for n, v in seen if n == "train/loss"]
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses)
    assert not torch.equal(step.learned_fx.raw.detach(), raw0) and torch.isfinite(step.learned_fx.raw).all()
    assert not torch.equal(next(step.model.parameters()).detach(), w0)
    assert step.learned_fx.raw.data_ptr() >= opt.flat_param.data_ptr()                  # re-homed in the flat buffer
    fb = [v for n, v in seen if n == "fx/flanger.feedback"]
    assert len(fb) == 3 and all(v.is_cuda and v.ndim == 0 for v in fb)                  # device scalars
    assert abs(float(fb[0]) - 0.3) < 1e-6 and float(fb[2]) != float(fb[0])
    for k in ("train/loss", "train/mrstft", "fx/flanger.feedback", "fx/flanger.depth", "fx/flanger.mix", "val/loss"):
        assert math.isfinite(hist[-1][k]), k
    # one needed name missing from the spec
    short = {"flanger": {k: v for k, v in spec["flanger"].items() if k != "width"}}
    bad = lightning.LFOExtractionThroughEffect(cnn(N), sr=SR, effect="flanger", learned_fx=short).to(dev).train()
    with pytest.raises(ValueError, match="flanger.width"):
        bad.training_step((dry, wet, None, None))


# ---- 7. every source of a constant in one batch ------------------------------------------------------------------------
SIX = FIVE + ("flanger",)
READERS = {"mix": ("delay", "tremolo", "phaser"), "one_minus_mix": ("delay", "tremolo"), "feedback": ("delay", "phaser"),
           "depth": ("delay", "phaser"), "lfo_scale": ("delay",), "min_delay": ("delay",), "centre_frequency_hz": ("phaser",)}
NAME_OF = {"mix": "mix", "one_minus_mix": "mix", "feedback": "feedback", "depth": "depth", "lfo_scale": "width",
           "min_delay": "min_delay_width", "centre_frequency_hz": "centre_frequency_hz"}
FAMILY = {"flanger": "delay", "chorus": "delay", "phaser": "phaser", "tremolo": "tremolo", "dry": "dry"}


def hand_constant(key, row, kind, table, values, fxp, counts):
    """One constant of one row by the stated rule.  A learned value (``values``: the launch's own fp32) and a batch tensor are
    fp32 and meet the row's fp32 sample count, or 1 - mix, in fp32; a fixed number and a python float are doubles, meet them in
    double and are rounded once.  Precedence: learned or fixed by ``table`` on the rows of its kind, else the batch."""
    name = NAME_OF[key]
    full = f"{kind}.{name}"
    if full in table.names:
        e = table.names.index(full)
        v = np.float32(values[e] if values.ndim == 1 else values[row, e])
    elif (kind, name) in table.fixed:
        v = float(table.fixed[(kind, name)])
    else:
        p = fxp[name]
        v = np.float32(p[row].item()) if isinstance(p, torch.Tensor) else float(p)
    count = {"lfo_scale": counts[0][row], "min_delay": counts[1][row]}.get(key)
    assert count is None or count.dtype == np.float32
    if isinstance(v, np.float32):
        out = v * count if count is not None else np.float32(1.0) - v if key == "one_minus_mix" else v
        assert out.dtype == np.float32
        return out
    return np.float32(v * float(count) if count is not None else 1.0 - v if key == "one_minus_mix" else v)


def check_constants(step, consts, values, fxp, B, dev):
    table = step.learned_fx if step.learned_fx is not None else step.fx_head
    m = step._mixed_rows(B, dev)
    counts = (m["max_lfo_delay"].cpu().numpy(), m["max_min_delay"].cpu().numpy())
    assert list(consts) == ["mix", "one_minus_mix", "feedback", "depth", "lfo_scale", "min_delay", "centre_frequency_hz"]
    values = values.cpu().numpy()
    for key, vec in consts.items():
        assert vec.shape == (B,) and vec.dtype == torch.float32 and vec.is_contiguous() and vec.device == dev
        rows = [i for i in range(B) if FAMILY[SIX[i]] in READERS[key]]
        want = torch.tensor(np.asarray([hand_constant(key, i, SIX[i], table, values, fxp, counts) for i in rows], dtype=np.float32))
        assert torch.equal(vec.cpu()[rows], want), (key, vec.cpu()[rows].tolist(), want.tolist())


def step_with(source, spec, dev):
    from mod_extraction_amd import lightning
    kw = {"learned_fx": spec} if source == "learned_fx" else {"fx_head": dict(spec, in_ch=8)}
    return lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect=SIX, **kw).to(dev)


@pytest.mark.parametrize("source", ["learned_fx", "fx_head"])
def test_every_source_in_one_batch(dev, source):
    B = 6
    g = torch.Generator().manual_seed(77)
    latent = torch.randn(B, 8, 4, generator=g).to(dev) if source == "fx_head" else None
    # flanger: width fixed, feedback and mix learned, the rest from the batch; chorus: the batch alone; phaser: the centre
    # fixed; tremolo: mix fixed
    spec = {"flanger": {"width": 0.8, "feedback": {"min": 0.0, "max": 0.7, "init": 0.3}, "mix": {"min": 0.0, "max": 1.0, "init": 0.4}},
            "phaser": {"centre_frequency_hz": 1300.1}, "tremolo": {"mix": 0.65}}
    step = step_with(source, spec, dev)
    fxp = {"feedback": (0.05 + 0.6 * torch.rand(B, generator=g)).to(dev), "min_delay_width": 0.37,
           "width": torch.rand(B, generator=g).to(dev), "depth": 0.9, "mix": torch.rand(B, generator=g).to(dev)}
    keep = {k: v.clone() for k, v in fxp.items() if isinstance(v, torch.Tensor)}
    consts = step.clip_constants(fxp, B, dev, latent)
    assert step._fx_values.shape == ((2,) if source == "learned_fx" else (B, 2))
    check_constants(step, consts, step._fx_values, fxp, B, dev)
    assert all(torch.equal(fxp[k], v) for k, v in keep.items())                         # the batch's tensors are not written
    # every name covered and no fx_params: the cached vectors, rewritten in place by the one launch
    full = {"flanger": dict(DELAY, width=0.8), "chorus": dict(DELAY, min_delay_width=0.25), "phaser": dict(ALL["phaser"], mix=0.9),
            "tremolo": {"mix": 0.65}}
    step = step_with(source, full, dev)
    first = step.clip_constants(None, B, dev, latent)
    check_constants(step, first, step._fx_values, None, B, dev)
    ptrs = {k: v.data_ptr() for k, v in first.items()}
    before = {k: v.clone() for k, v in first.items()}
    with torch.no_grad():
        (step.learned_fx.raw if source == "learned_fx" else step.fx_head.bias).add_(0.3)
    second = step.clip_constants(None, B, dev, latent)
    assert {k: v.data_ptr() for k, v in second.items()} == ptrs
    check_constants(step, second, step._fx_values, None, B, dev)
    assert not torch.equal(second["feedback"], before["feedback"]) and torch.equal(first["feedback"], second["feedback"])

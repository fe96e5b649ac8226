"""GPU: lightning.LFOExtractionThroughEffect(fx_head=...) -- effect parameters per clip, predicted by fx.FxParamHead from the
model's latent (csrc/fx_head.hip).  Except in 5 the model is a stub that returns a given (lfo, latent) pair of leaf tensors.

1. zero-weight identity: B = 6, N = 22 272, the kinds and batch of test_consistency_with_the_unlearned_step.  The fx_head
   step with weight = 0 and a spread bias against the learned_fx step with raw = bias: wet_hat, loss and d loss / d LFO are
   torch.equal; latent.grad is exactly 0; bias.grad and weight.grad against the helper's sums over the adjoints' own (6, B)
   buffer (bias.grad also against raw.grad): |got - want| <= 6e-8 |want| + 1e-12 sum |terms|, one fp32 cast of an fp64 sum.
2. per-row consistency: a non-zero weight gives the rows of one kind different values (asserted).  The kernel's values, put
   into plain (B,) fx_params tensors and run through a step with neither learned_fx nor fx_head, give the same wet_hat, loss
   and d loss / d LFO, torch.equal; so do render(..., latent=) and the no-grad branch; the batch's own tensors are not written.
3. end-to-end gradient against fp64: B = 5, one row per kind, N = 4096, n_mod = 17, C = 8, W = 17, {"l1": 1.0}: the recipe of
   test_parameter_gradient_against_fp64 (the fp64 adjoint helpers fed the step's own dy), chained through
   tests/helpers/fx_head64.py.  That test holds a per-clip parameter gradient g to max |difference| over the rows of a launch
   <= gate * max |reference| over them (1e-5 flanger / chorus / tremolo, 1.8e-4 phaser).  bias.grad, weight.grad and
   latent.grad are linear in those g, so the same gate is carried through the chain term by term:
       |d bias[e]|  error <= gate N_e |k_e|,  |d weight[e, c]| <= gate N_e |k_e pooled[row_e, c]|,
       |d latent[b, c, w]| <= gate sum_(e of row b) N_e |k_e weight[e, c]| / W,
   N_e = max |reference| over the launch's rows of entry e's parameter, k_e = sample count * d value / d raw (exact in fp64).
4. it fits per clip, which no shared value can: B = 8 flanger clips, true feedback 0.15 on the even and 0.55 on the odd rows,
   everything else fixed at its truth, the LFO held at the label, a latent that is +-1 in channel 0 by group; wet rendered by a
   plain step from per-row fx_params.  80 Adam steps on the head: final loss < first loss, each group's mean predicted
   feedback closer to its truth than at the start, even mean < odd mean (values and ratios are printed, not gated further).
5. real shape: Spectral2DCNN, (dry, wet, None, None) batches, three trainer.Trainer steps through a stub data module: finite
   losses; fx_head.bias, fx_head.weight and the extractor's first convolution weight all moved; fx/flanger.feedback and
   fx_std/flanger.feedback among the logged metrics; a checkpoint written and read back restores fx_head.weight bit for
   bit; with one needed name uncovered the step raises a ValueError that names it."""
import math

import numpy as np
import pytest
import torch

from tests.helpers import fx_head64 as hh
from tests.helpers import fx_params64 as h
from tests.helpers.flanger_adjoint64_lr import flanger_adjoint64_lr
from tests.helpers.tremolo_adjoint64 import tremolo_adjoint64
from tests.test_gpu_learned_fx_step import ALL, FIVE, SR, PairStub, smooth_lfo
from tests.test_gpu_mixed_step import batch_of, cnn
from tests.test_gpu_phaser_grad import gpu_decisions, reference

pytestmark = pytest.mark.gpu


class Pair(torch.nn.Module):
    """A model that returns a given (lfo (B, 1, n), latent (B, C, W)) pair of leaf tensors, whatever it is fed."""

    def __init__(self, lfo, latent):
        super().__init__()
        self.lfo, self.latent = lfo, latent

    def forward(self, x):
        return self.lfo, self.latent


def set_head(head, weight, bias):
    with torch.no_grad():
        head.weight.copy_(torch.as_tensor(weight, dtype=torch.float32))
        head.bias.copy_(torch.as_tensor(bias, dtype=torch.float32))


def spy_on_backward(head, seen):
    """Keep what the head's backward launch is given: the adjoints' (6, B) buffer, raw_rows and pooled."""
    orig = head.backward_rows

    def spy(grads, raw_rows, pooled, *a, **k):
        seen.update(grads=grads.clone(), raw_rows=raw_rows.clone(), pooled=pooled.clone())
        return orig(grads, raw_rows, pooled, *a, **k)

    head.backward_rows = spy


def table(head):
    f, i = head.tab_f.cpu().numpy(), head.tab_i.cpu().numpy()
    return f[0], f[1], i[0], i[1], i[2]


def worst_ratio(got, want, terms, rel=6e-8, floor=1e-12):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    return float((err / np.maximum(np.abs(want) + (floor / rel) * terms, 1e-300)).max())


def consistency_batch(dev):
    from mod_extraction_amd.util import linear_interpolate_last_dim
    kinds = FIVE + ("flanger",)
    B, N, n_frames = 6, 22272, 88
    dry, wet, mod, _ = batch_of(dev, kinds, B, N, 21, fixed_lead=0)
    t = torch.linspace(0.0, 1.0, n_frames, device=dev)
    bump = 0.1 * torch.sin(2 * math.pi * (1.5 * t[None, :] + torch.arange(B, device=dev)[:, None] / B))
    h0 = (linear_interpolate_last_dim(mod, n_frames, align_corners=True) + bump).clamp(0.0, 1.0)
    g = torch.Generator().manual_seed(8)
    latent = torch.randn(B, 8, 17, generator=g).to(dev)
    return kinds, B, dry, wet, h0, latent


def test_zero_weight_identity(dev):
    from mod_extraction_amd import fx, lightning
    kinds, B, dry, wet, h0, latent = consistency_batch(dev)
    weights = {"mrstft": 1.0, "l1": 0.5}
    la, lb = (h0.clone().unsqueeze(1).requires_grad_(True) for _ in range(2))
    za = latent.clone().requires_grad_(True)
    headed = lightning.LFOExtractionThroughEffect(Pair(la, za), sr=SR, effect=kinds, audio_loss_dict=weights,
                                                  fx_head=fx.FxParamHead(ALL, in_ch=8)).to(dev)
    learned = lightning.LFOExtractionThroughEffect(Pair(lb, latent), sr=SR, effect=kinds, audio_loss_dict=weights,
                                                   learned_fx=ALL).to(dev)
    head, lf = headed.fx_head, learned.learned_fx
    bias = np.random.default_rng(5).uniform(-2.0, 2.0, 15)
    set_head(head, torch.zeros(15, 8), bias)
    with torch.no_grad():
        lf.raw.copy_(head.bias)
    seen = {}
    spy_on_backward(head, seen)
    loss_a, da, _ = headed.common_step((dry, wet, None, None), is_training=True)
    loss_a.backward()
    loss_b, db, _ = learned.common_step((dry, wet, None, None), is_training=True)
    loss_b.backward()
    assert float(loss_a.detach()) > 0 and float(la.grad.abs().max()) > 0 and not torch.equal(da["wet_hat"][:4], dry[:4])
    assert torch.equal(da["wet_hat"], db["wet_hat"]) and torch.equal(loss_a.detach(), loss_b.detach())
    assert torch.equal(la.grad, lb.grad)
    assert da["fx_values"].shape == (B, 15) and torch.equal(da["fx_values"], learned._fx_values.expand(B, 15))
    assert za.grad is not None and za.grad.shape == za.shape and bool((za.grad == 0).all())
    # the sums of mx_fx_head_bwd over the adjoints' own buffer, restated in fp64
    lo, hi, is_log, slot, kind = table(head)
    m = headed._mixed_rows(B, dev)
    want = hh.backward(seen["grads"].cpu().numpy(), seen["raw_rows"].double().cpu().numpy(),
                       seen["pooled"].double().cpu().numpy(), np.zeros((15, 8)), lo, hi, is_log, slot, kind, 1.0,
                       m["row_kind"].cpu().numpy(), m["max_lfo_delay"].cpu().numpy(), m["max_min_delay"].cpu().numpy(), 17)
    assert np.isfinite(want["d_bias"]).all() and (want["d_bias"] != 0).all()
    r = worst_ratio(head.bias.grad.cpu().numpy(), want["d_bias"], want["abs_d_bias"])
    print(f"bias.grad against the helper: worst error / (|want| + 1.67e-5 sum |terms|) {r:.3e}")
    assert r <= 6e-8
    r = worst_ratio(head.bias.grad.cpu().numpy(), lf.raw.grad.double().cpu().numpy(), want["abs_d_bias"])
    print(f"bias.grad against raw.grad: worst error / (|want| + 1.67e-5 sum |terms|) {r:.3e}; "
          f"{int((head.bias.grad != lf.raw.grad).sum())} of 15 differ in their bits")
    assert r <= 6e-8
    r = worst_ratio(head.weight.grad.cpu().numpy(), want["d_weight"], want["abs_d_weight"])
    print(f"weight.grad against the outer-product restatement: worst error / (|want| + 1.67e-5 sum |terms|) {r:.3e}; "
          f"max |want| {np.abs(want['d_weight']).max():.3e}")
    assert r <= 6e-8 and float(head.weight.grad.abs().max()) > 0


def test_per_row_consistency(dev):
    from mod_extraction_amd import fx, lightning
    kinds, B, dry, wet, h0, latent = consistency_batch(dev)
    weights = {"mrstft": 1.0, "l1": 0.5}
    la, lb = (h0.clone().unsqueeze(1).requires_grad_(True) for _ in range(2))
    headed = lightning.LFOExtractionThroughEffect(Pair(la, latent), sr=SR, effect=kinds, audio_loss_dict=weights,
                                                  fx_head=fx.FxParamHead(ALL, in_ch=8)).to(dev)
    plain = lightning.LFOExtractionThroughEffect(Pair(lb, latent), sr=SR, effect=kinds, audio_loss_dict=weights)
    head = headed.fx_head
    g = np.random.default_rng(6)
    set_head(head, g.normal(0.0, 1.5, (15, 8)), g.uniform(-1.0, 1.0, 15))
    loss_a, da, _ = headed.common_step((dry, wet, None, None), is_training=True)
    loss_a.backward()
    values = da["fx_values"]
    assert values.shape == (B, 15) and values.dtype == torch.float32
    spread = (values[0] - values[5]).abs()                                              # rows 0 and 5 are both flanger rows
    print(f"flanger entries of rows 0 and 5 differ by {[round(float(v), 4) for v in spread[:5]]}")
    assert bool((spread[:5] > 1e-3).all())
    names = head.names
    fxp = {}
    for name in ("feedback", "min_delay_width", "width", "depth", "mix", "centre_frequency_hz"):
        rows = [values[b, names.index(f"{k}.{name}")] if f"{k}.{name}" in names else torch.tensor(0.5, device=dev)
                for b, k in enumerate(kinds)]
        fxp[name] = torch.stack(rows).contiguous()
    loss_b, db, _ = plain.common_step((dry, wet, None, fxp), is_training=True)
    loss_b.backward()
    hat = da["wet_hat"]
    print(f"consistency: loss {float(loss_a):.6e} / {float(loss_b):.6e}, {int((hat != db['wet_hat']).sum())} of {hat.numel()} "
          f"samples and {int((la.grad != lb.grad).sum())} of {la.grad.numel()} gradient values differ")
    assert float(loss_a) > 0 and float(la.grad.abs().max()) > 0 and not torch.equal(hat[:4], dry[:4])
    assert torch.equal(hat, db["wet_hat"]) and torch.equal(loss_a.detach(), loss_b.detach()) and torch.equal(la.grad, lb.grad)
    assert torch.equal(hat[4], dry[4]) and bool((la.grad[4] == 0).all())                # the dry row
    assert all(torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0 for p in (head.weight, head.bias))
    # render() and the no-grad branch predict from the latent too (the forward kernel alone)
    assert torch.equal(headed.render(dry, h0, None, latent=latent), hat)
    loss_v, dv, _ = headed.validation_step((dry, wet, None, None))
    assert torch.equal(dv["wet_hat"], hat) and torch.equal(dv["fx_values"], values) and loss_v.grad_fn is None
    with pytest.raises(ValueError, match="latent"):
        headed.render(dry, h0, None)
    # precedence: a batch that carries fx_params is overridden on the predicted rows -- here on all of them
    other = {k: torch.full((B,), 0.123, device=dev) for k in fxp}
    keep = {k: v.clone() for k, v in other.items()}
    assert torch.equal(headed.render(dry, h0, other, latent=latent), hat)
    assert all(torch.equal(other[k], keep[k]) for k in other)                           # and the batch's tensors are not written


def test_gradient_against_fp64(dev):
    from mod_extraction_amd import fx, lightning
    from mod_extraction_amd.effect_losses import effect_loss_grad
    B, N, n_mod, C, W = 5, 4096, 17, 8, 17
    g = torch.Generator().manual_seed(44)
    dry = (0.3 * torch.randn(B, 1, N, generator=g)).to(dev)
    wet = (0.3 * torch.randn(B, 1, N, generator=g)).to(dev)
    latent = torch.randn(B, C, W, generator=g).to(dev).requires_grad_(True)
    hl = smooth_lfo(dev, B, n_mod, 10).unsqueeze(1).requires_grad_(True)
    step = lightning.LFOExtractionThroughEffect(Pair(hl, latent), sr=SR, effect=FIVE, audio_loss_dict={"l1": 1.0},
                                                fx_head=fx.FxParamHead(ALL, in_ch=C, raw_gain=2.0)).to(dev)
    head = step.fx_head
    rng = np.random.default_rng(9)
    set_head(head, rng.normal(0.0, 0.5, (15, C)), rng.uniform(-0.5, 0.5, 15))
    loss, dd, _ = step.common_step((dry, wet, None, None), is_training=True)
    loss.backward()
    wet_hat = dd["wet_hat"]
    pooled, raw_rows = (t.double().cpu().numpy() for t in step._head_rows)
    got_b, got_w = head.bias.grad.double().cpu().numpy(), head.weight.grad.double().cpu().numpy()
    got_l = latent.grad.double().cpu().numpy()
    assert got_l.shape == (B, C, W) and all(np.isfinite(a).all() for a in (got_b, got_w, got_l))
    assert np.array_equal(got_l, np.repeat(got_l[:, :, :1], W, axis=2)) and not got_l[4].any()
    assert float(np.abs(raw_rows).max()) < 3.0                                          # away from saturation: k_e is not tiny
    consts = {k: v.clone() for k, v in step.clip_constants(None, B, dev, latent).items()}
    dy = effect_loss_grad(wet_hat, wet, {"l1": 1.0}, **step._grad_modules())
    x_np, dy_np, mod_np = dry[:, 0].cpu().numpy(), dy.cpu().numpy(), hl.detach()[:, 0].cpu().numpy()
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
    _, st, mod_g = fx.phaser_forward_stash_lr(dry[2:3, 0].contiguous(), pc, None, SR, N, hl.detach()[2:3, 0].contiguous())
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
    # the (6, B) buffer of the references (NaN wherever no entry reads), chained through the helper
    lo, hi, is_log, slot, kind = table(head)
    G = np.full((6, B), np.nan)
    for (s, r), v in ref.items():
        G[h.SLOTS.index(s), r] = v
    rk, ml, mm = (m[k].cpu().numpy() for k in ("row_kind", "max_lfo_delay", "max_min_delay"))
    w64 = head.weight.detach().double().cpu().numpy()
    want = hh.backward(G, raw_rows, pooled, w64, lo, hi, is_log, slot, kind, head.raw_gain, rk, ml, mm, W)
    # N_e: max |reference| over the rows of the launch (the flanger and the chorus row are one launch), k_e, the gate
    gate_of = {"flanger": 1e-5, "chorus": 1e-5, "tremolo": 1e-5, "phaser": 1.8e-4}
    k_e, n_e, gate, row_e = np.zeros(15), np.zeros(15), np.zeros(15), np.zeros(15, dtype=int)
    for e, full in enumerate(head.names):
        kd, name = full.split(".")
        row, s = FIVE.index(kd), h.NAME_SLOT[name]
        count = ml[row] if s == "lfo_scale" else mm[row] if s == "min_delay" else 1.0
        dv = h.dvalue_draw(raw_rows[row, e:e + 1], lo[e:e + 1], hi[e:e + 1], is_log[e:e + 1], head.raw_gain)[0]
        rows = (0, 1) if kd in ("flanger", "chorus") else (row,)
        k_e[e], n_e[e], gate[e], row_e[e] = count * dv, max(abs(ref[(s, r)]) for r in rows), gate_of[kd], row
        print(f"{full}: d loss / d bias {got_b[e]:+.6e}, fp64 {want['d_bias'][e]:+.6e}")
    unit = n_e * np.abs(k_e)                                                            # the error of d_raw[row_e, e] per unit gate
    worst = {"flanger": 0.0, "chorus": 0.0, "tremolo": 0.0, "phaser": 0.0}
    for e, full in enumerate(head.names):
        kd = full.split(".")[0]
        rb = abs(got_b[e] - want["d_bias"][e]) / unit[e]
        rw = float((np.abs(got_w[e] - want["d_weight"][e]) / (unit[e] * np.abs(pooled[row_e[e]]))).max())
        worst[kd] = max(worst[kd], rb, rw)
        assert rb <= gate[e] and rw <= gate[e], full
    print("bias.grad / weight.grad, worst error in units of N_e |k_e| (x |pooled|):", {k: f"{v:.2e}" for k, v in worst.items()})
    worst_l = {}
    for b, kd in enumerate(FIVE[:4]):
        es = [e for e in range(15) if row_e[e] == b]
        bound = sum(unit[e] * np.abs(w64[e]) for e in es) / W                           # (C,), per unit gate
        worst_l[kd] = float((np.abs(got_l[b, :, 0] - want["d_latent"][b]) / bound).max())
        assert worst_l[kd] <= gate_of[kd], kd
    print("latent.grad, worst error in units of sum_e N_e |k_e weight[e, c]| / W:", {k: f"{v:.2e}" for k, v in worst_l.items()})


def test_it_fits_per_clip(dev):
    from mod_extraction_amd import fx, lightning
    B, N = 8, 22272
    dry, _, mod, _ = batch_of(dev, ("flanger",), B, N, 31)
    truth = torch.tensor([0.15, 0.55] * (B // 2), device=dev)
    fixed = {"min_delay_width": 1.0, "width": 1.0, "depth": 1.0, "mix": 1.0}
    plain = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect="flanger", max_lfo_delay_ms=4.0)
    wet = plain.render(dry, mod, dict(fixed, feedback=truth))
    latent = torch.zeros(B, 4, 5, device=dev)
    latent[0::2, 0], latent[1::2, 0] = -1.0, 1.0                                        # channel 0 marks the group
    spec = {"flanger": dict(fixed, feedback={"min": 0.0, "max": 0.95, "init": 0.35})}
    step = lightning.LFOExtractionThroughEffect(Pair(mod.unsqueeze(1), latent), sr=SR, effect="flanger", max_lfo_delay_ms=4.0,
                                                fx_head=fx.FxParamHead(spec, in_ch=4)).to(dev).train()
    head = step.fx_head
    opt = torch.optim.Adam(head.parameters(), lr=0.05)
    batch = (dry, wet, None, None)
    losses, start = [], None
    for _ in range(80):
        opt.zero_grad()
        loss, dd, _ = step.common_step(batch, is_training=True)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
        if start is None:
            start = dd["fx_values"][:, 0].clone()
    with torch.no_grad():
        final, dd, _ = step.common_step(batch, is_training=False)
    end = dd["fx_values"][:, 0]
    first, final = float(losses[0]), float(final)
    even0, odd0, even1, odd1 = (float(v) for v in (start[0::2].mean(), start[1::2].mean(), end[0::2].mean(), end[1::2].mean()))
    print(f"per-clip fit: loss {first:.6e} -> {final:.6e}, ratio {final / first:.4f}")
    print(f"  even rows (truth 0.15): {even0:.4f} -> {even1:.4f}, distance ratio {abs(even1 - 0.15) / abs(even0 - 0.15):.4f}")
    print(f"  odd rows  (truth 0.55): {odd0:.4f} -> {odd1:.4f}, distance ratio {abs(odd1 - 0.55) / abs(odd0 - 0.55):.4f}")
    assert abs(even0 - 0.35) < 1e-6 and abs(odd0 - 0.35) < 1e-6                         # a fresh head predicts init everywhere
    assert final < first
    assert abs(even1 - 0.15) < abs(even0 - 0.15) and abs(odd1 - 0.55) < abs(odd0 - 0.55)
    assert even1 < odd1
    assert float(head.weight.detach()[0, 1:].abs().max()) == 0.0                        # the silent channels got no gradient


def test_real_shape(dev, tmp_path):
    from mod_extraction_amd import lightning, optim, trainer
    B, N = 4, 22272
    dry, wet, _, _ = batch_of(dev, ("flanger",), B, N, 41)
    spec = {"flanger": {"feedback": {"min": 0.0, "max": 0.95, "init": 0.3}, "depth": {"min": 0.0, "max": 1.0, "init": 0.5},
                        "mix": 1.0, "width": 1.0, "min_delay_width": 0.5}}
    torch.manual_seed(4)
    step = lightning.LFOExtractionThroughEffect(cnn(N), sr=SR, effect="flanger", fx_head=spec).to(dev).train()
    head = step.fx_head
    assert head.in_ch == 64 and not bool(head.weight.any())
    opt = optim.FlatAdamW(step.parameters(), lr=1e-4, betas=(0.8, 0.99))
    b0, w0 = head.bias.detach().clone(), head.weight.detach().clone()
    c0 = next(step.model.parameters()).detach().clone()
    seen = []
    keep = step.log
    step.log = lambda n, v: (seen.append((n, v)), keep(n, v))[1]
    hist = trainer.Trainer(max_epochs=1, log_fn=None).fit(step, PairStub(dry, wet), opt)
    losses = [float(v) for n, v in seen if n == "train/loss"]
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses)
    assert not torch.equal(head.bias.detach(), b0) and not torch.equal(head.weight.detach(), w0)
    assert torch.isfinite(head.bias).all() and torch.isfinite(head.weight).all()
    assert not torch.equal(next(step.model.parameters()).detach(), c0)
    for p in (head.weight, head.bias):                                                  # re-homed in the flat buffer
        assert opt.flat_param.data_ptr() <= p.data_ptr() < opt.flat_param.data_ptr() + 4 * opt.flat_param.numel()
    fb = [v for n, v in seen if n == "fx/flanger.feedback"]
    sd = [v for n, v in seen if n == "fx_std/flanger.feedback"]
    assert len(fb) == len(sd) == 3 and all(v.is_cuda and v.ndim == 0 for v in fb + sd)  # device scalars
    assert abs(float(fb[0]) - 0.3) < 1e-6 and float(sd[0]) == 0.0                       # a fresh head: init on every row
    assert float(fb[2]) != float(fb[0]) and float(sd[2]) > 0.0
    for k in ("train/loss", "train/mrstft", "fx/flanger.feedback", "fx/flanger.depth", "fx_std/flanger.feedback",
              "fx_std/flanger.depth", "val/loss"):
        assert math.isfinite(hist[-1][k]), k
    # a checkpoint written and read back
    path = str(tmp_path / "head.ckpt")
    trainer.save_checkpoint(path, step, opt, 0, 3)
    torch.manual_seed(5)
    again = lightning.LFOExtractionThroughEffect(cnn(N), sr=SR, effect="flanger", fx_head=spec).to(dev)
    assert not torch.equal(again.fx_head.weight, head.weight)
    blob = trainer.resume_from_checkpoint(path, again, None)
    assert "fx_head.weight" in blob["state_dict"] and "fx_head.bias" in blob["state_dict"]
    again.load_state_dict(blob["state_dict"], strict=True)
    assert torch.equal(again.fx_head.weight, head.weight) and torch.equal(again.fx_head.bias, head.bias)
    # one needed name uncovered
    short = {"flanger": {k: v for k, v in spec["flanger"].items() if k != "width"}}
    bad = lightning.LFOExtractionThroughEffect(cnn(N), sr=SR, effect="flanger", fx_head=short).to(dev).train()
    with pytest.raises(ValueError, match="flanger.width"):
        bad.training_step((dry, wet, None, None))

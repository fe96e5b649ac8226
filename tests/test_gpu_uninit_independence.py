"""No op may depend on the contents of uninitialised device memory.

The Python wrappers allocate their outputs, operands and workspaces with ``torch.empty`` and its variants.  A short test
process nearly always gets fresh, zero-filled memory from the caching allocator; a training run gets the previous step's
gradients, index words and f16 operands.  Every case here runs the same product wrapper (forward and backward) three times
under ``tests/helpers/poison_alloc.poisoned``: with every such buffer pre-filled with pattern ``A`` (0.0 / 0), ``B`` (0.5 / 1)
and ``C`` (NaN / 1), in that order.  A kernel that reads a pitch-padding column, a halo row or a workspace word its producer
never wrote, or that accumulates into an output it was supposed to overwrite, gives results that differ between the runs.

Per case:
  * every public output and every gradient is bit-identical (``torch.equal``) across the runs -- the kernels are
    deterministic.  ``B`` is compared with ``A`` first and fails there; ``C`` only runs for a case whose in-range patterns agree;
  * no NaN in any of them under ``C``;
  * the poison counter is non-zero and names the wrapper functions the case is meant to reach, so a case that stops going
    through ``torch.empty`` fails instead of passing vacuously.

Inputs, parameters and seeds are made on the CPU, outside the context.  Whole outputs are compared; the only exemption is a
region an existing docstring declares unspecified in words (quoted where it is used).
``test_sensitivity_control_tremolo_backward_zero_fill`` shows that the probe sees a zero-fill that IS needed.

MODEX_POISON_REPORT=<file>: every run appends its call-site table (with line numbers) as a JSON line.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers.poison_alloc import poisoned

pytestmark = pytest.mark.gpu

PKG = "mod_extraction_amd."
SR = 44100.0
_REPORT = os.environ.get("MODEX_POISON_REPORT")


# ---------------------------------------------------------------------------------------------------------------------
# the probe
# ---------------------------------------------------------------------------------------------------------------------
def _snapshot(out):
    snap = {}
    for k, v in out.items():
        if v is None:
            continue
        assert isinstance(v, torch.Tensor), (k, type(v))
        snap[k] = v.detach().cpu().clone()
    return snap


def run_patterns(case, expect, patterns=("A", "B", "C"), forbid=()):
    """``case()`` -> {name: tensor} under each pattern in turn; asserts as the module docstring says.  ``expect``: the
    "module:function" call sites (without the package prefix) the case must reach; ``forbid``: sites it must not."""
    first, tables = None, {}
    for pat in patterns:
        with poisoned(pat) as ctx:
            out = case()
            torch.cuda.synchronize()
        snap = _snapshot(out)
        tables[pat] = dict(ctx.sites)
        if _REPORT:
            with open(_REPORT, "a") as f:
                f.write(json.dumps({"test": os.environ.get("PYTEST_CURRENT_TEST", ""), "pattern": pat, "sites": dict(ctx.sites),
                                    "lines": dict(ctx.lines)}) + "\n")
        assert ctx.total >= 1, "the case allocated nothing through torch.empty: it checks nothing"
        missing = sorted(PKG + e for e in expect if PKG + e not in ctx.sites)
        assert not missing, f"pattern {pat}: call sites not reached {missing}; reached {sorted(ctx.sites)}"
        present = sorted(PKG + e for e in forbid if PKG + e in ctx.sites)
        assert not present, f"pattern {pat}: call sites that should not allocate here {present}"
        if pat == "C":
            for k, v in snap.items():
                if v.is_floating_point():
                    assert not bool(torch.isnan(v).any()), f"{k}: NaN under pattern C (sites {sorted(ctx.sites)})"
        if first is None:
            first = snap
            continue
        assert set(snap) == set(first)
        for k, v in snap.items():
            same = v.shape == first[k].shape and v.dtype == first[k].dtype and torch.equal(v, first[k])
            if not same:
                diff = (v != first[k]) if v.shape == first[k].shape else None
                n_bad = "shape" if diff is None else int(diff.sum())
                where = "" if diff is None or diff.ndim == 0 else f", first at {tuple(int(i) for i in diff.nonzero()[0])}"
                raise AssertionError(f"{k}: pattern {pat} differs from pattern {patterns[0]} in {n_bad} of {v.numel()} elements"
                                     f"{where}; poisoned call sites: {sorted(ctx.sites)}")
    return tables


def _rng(seed):
    return np.random.default_rng(seed)


def _dv(dev, a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def _audio(B, n, seed, ch=None):
    """White noise plus a tone per row, in (-1, 1): (B, n) or (B, ch, n) on the host."""
    r = _rng(seed)
    shape = (B, n) if ch is None else (B, ch, n)
    t = np.arange(n) / SR
    f = 180.0 + 400.0 * r.random(shape[:-1] + (1,))
    return (0.55 * (2 * r.random(shape) - 1) + 0.4 * np.sin(2 * np.pi * f * t)).astype(np.float32)


def _lfo_rows(B, n, seed, lo=0.6, hi=5.0, dur=2.0):
    """(B, n) cosine LFOs in [0, 1] with a few periods over the row."""
    r = _rng(seed)
    t = np.linspace(0.0, dur, n)
    f = lo + (hi - lo) * r.random((B, 1))
    ph = 2 * np.pi * r.random((B, 1))
    return (0.5 + 0.5 * np.cos(2 * np.pi * f * t + ph)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# CNN stack
# ---------------------------------------------------------------------------------------------------------------------
CNN_CFG = dict(in_ch=2, n_fft=1024, hop_len=256, n_mels=64, kernel_size=(5, 13), out_channels=[64] * 6,
               temp_dilations=[1, 1, 2, 4, 8, 16], pool_size=(2, 1), latent_dim=1, freq_mask_amount=0.25,
               time_mask_amount=0.25, use_ln=True)
MASKS = (3, 11, 20, 41)
KNOBS = ["GPOOL_FUSED", "STATS_FUSED", "LN_FUSED", "WGRAD_SPARSE", "DGRAD_SPARSE", "BLOCK1_PAIR", "BLOCK1_F16"]   # tests/test_gpu_cnn.py
CNN_SITES_F32 = {"models:log_mel", "models:_f32", "models:_block_fwd", "models:_head_bwd", "models:_wgrad_part"}
CNN_SITES_F16 = CNN_SITES_F32 | {"models:_f16_pair", "models:_wgrad_f16x3"}
FRESH_GRADS = "models:weight"                      # _ParamGrads.weight: a fresh tensor per weight gradient


def _cnn_model(dev, n_samples, seed=0, **over):
    from mod_extraction_amd import models as amodels
    torch.manual_seed(seed)
    m = amodels.Spectral2DCNN(**dict(CNN_CFG, n_samples=n_samples, **over))
    with torch.no_grad():                       # PReLU slopes away from their trivial init, as tests/test_gpu_cnn.py does
        for layer in m.cnn:
            if isinstance(layer, torch.nn.PReLU):
                layer.weight.uniform_(0.05, 0.45)
    assert not m.generic
    return m.to(dev).eval()


def _cnn_inputs(dev, B, n, ch=2, seed=1, latent_ch=64):
    x = _dv(dev, _audio(B, n, seed, ch=ch))
    wl = _dv(dev, _rng(seed + 1).random((B, latent_ch, n // 256 + 1)) - 0.5)
    return x, wl


def _cnn_case(model, x, wl, masks=MASKS):
    def case():
        model.zero_grad(set_to_none=True)
        out, latent = model(x, masks)
        (out.sum() + (latent * wl).sum()).backward()
        res = {"out": out, "latent": latent}
        for name, p in model.named_parameters():
            assert p.grad is not None, name
            res["grad/" + name] = p.grad
        return res
    return case


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_cnn_stack(dev, precision):
    model = _cnn_model(dev, 22272)
    model.conv_precision = precision
    x, wl = _cnn_inputs(dev, 3, 22272)
    run_patterns(_cnn_case(model, x, wl), (CNN_SITES_F16 if precision == "f16x3" else CNN_SITES_F32) | {FRESH_GRADS})


@pytest.mark.parametrize("knob", KNOBS)
def test_cnn_stack_with_a_fusion_switched_off(dev, knob, monkeypatch):
    """Every knob changes which buffers exist (tests/test_gpu_cnn.py has the list and what each one selects)."""
    from mod_extraction_amd import models as amodels
    monkeypatch.setattr(amodels, knob, False)
    model = _cnn_model(dev, 22272)
    x, wl = _cnn_inputs(dev, 3, 22272)
    run_patterns(_cnn_case(model, x, wl), CNN_SITES_F16 | {FRESH_GRADS})


def test_cnn_stack_single_channel_input(dev):
    model = _cnn_model(dev, 22272, in_ch=1)
    x, wl = _cnn_inputs(dev, 3, 22272, ch=1)
    run_patterns(_cnn_case(model, x, wl), CNN_SITES_F16)


def test_cnn_stack_second_backward_through_a_retained_graph(dev):
    """The second backward finds the kept operand pairs gone and derives them again (models._CNNStack.backward)."""
    model = _cnn_model(dev, 22272)
    x, wl = _cnn_inputs(dev, 3, 22272)

    def case():
        model.zero_grad(set_to_none=True)
        out, latent = model(x, MASKS)
        loss = out.sum() + (latent * wl).sum()
        loss.backward(retain_graph=True)
        res = {"out": out, "latent": latent}
        res.update({"grad1/" + n: p.grad for n, p in model.named_parameters()})
        model.zero_grad(set_to_none=True)
        loss.backward()
        res.update({"grad2/" + n: p.grad for n, p in model.named_parameters()})
        return res

    run_patterns(case, CNN_SITES_F16 | {FRESH_GRADS})


@pytest.mark.parametrize("direct", [True, False], ids=["flat-buffer", "fresh-tensors"])
def test_cnn_stack_direct_grads_on_and_off(dev, direct, monkeypatch):
    """DIRECT_GRADS on: the gradients are written in place into FlatAdamW's flat buffer (built inside the context, so the
    buffer's own allocation is poisoned before first use); off: into fresh tensors that autograd accumulates."""
    from mod_extraction_amd import models as amodels, optim
    monkeypatch.setattr(amodels, "DIRECT_GRADS", direct)
    model = _cnn_model(dev, 22272)
    x, wl = _cnn_inputs(dev, 3, 22272)

    def case():
        opt = optim.FlatAdamW(model.parameters(), lr=1e-4, betas=(0.8, 0.99))
        opt.zero_grad()
        out, latent = model(x, MASKS)
        with opt.direct_backward():
            (out.sum() + (latent * wl).sum()).backward()
        return {"out": out, "latent": latent, "flat_grad": opt.flat_grad, "flat_param": opt.flat_param}

    if direct:
        run_patterns(case, CNN_SITES_F16 | {"optim:__init__"}, forbid={FRESH_GRADS})
    else:
        run_patterns(case, CNN_SITES_F16 | {"optim:__init__", FRESH_GRADS})


def test_cnn_stack_shipped_frame_count(dev):
    """345 frames: 7 padding columns in every 352-pitch row."""
    model = _cnn_model(dev, 88200)
    assert model.n_frames == 345
    x, wl = _cnn_inputs(dev, 2, 88200)
    run_patterns(_cnn_case(model, x, wl), CNN_SITES_F16 | {FRESH_GRADS})


# ---------------------------------------------------------------------------------------------------------------------
# generic routes
# ---------------------------------------------------------------------------------------------------------------------
def test_generic_cnn(dev):
    """tests/test_gpu_generic_cnn.py "pool1-1x1" and "3x5-mixed-channels": its smallest configurations."""
    from mod_extraction_amd import models as amodels
    for cfg in (dict(in_ch=1, n_samples=6000, n_mels=24, kernel_size=(1, 1), out_channels=[4, 6], pool_size=(1, 1)),
                dict(in_ch=3, n_samples=12000, n_mels=60, kernel_size=(3, 5), out_channels=[8, 12, 20],
                     bin_dilations=[1, 2, 1], temp_dilations=[1, 3, 5], pool_size=(3, 1), latent_dim=2)):
        torch.manual_seed(0)
        model = amodels.Spectral2DCNN(**cfg)
        assert model.generic
        model = model.to(dev).eval()
        n = cfg["n_samples"]
        x = _dv(dev, _audio(3, n, 2, ch=cfg["in_ch"]))
        wl = _dv(dev, _rng(3).random((3, cfg["out_channels"][-1], n // 256 + 1)) - 0.5)
        run_patterns(_cnn_case(model, x, wl, masks=(0, 0, 0, 0)), {"models:log_mel", "cnn_generic:_empty"})


def test_general_tcn(dev):
    """tests/test_tcn_general.py "padded" (tests/golden/make_golden_tcn_general.py): its smallest trainable configuration."""
    from mod_extraction_amd import tcn
    torch.manual_seed(0)
    net = tcn.TCN(out_channels=[8, 8], dilations=[1, 3], in_ch=4, kernel_size=5, padding=1, is_causal=False).to(dev).train()
    x0 = _dv(dev, _rng(4).standard_normal((2, 4, 64)))

    def case():
        net.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = net(x, None)
        wy = torch.linspace(0.5, 1.5, y.numel(), device=dev).view_as(y)
        (y * wy).sum().backward()
        res = {"y": y, "dx": x.grad}
        res.update({"grad/" + n: p.grad for n, p in net.named_parameters()})
        return res

    run_patterns(case, {"tcn:_f32"})


def test_spectral_tcn(dev):
    """The fused TCN stack behind models.SpectralTCN (tests/test_tcn.py's small configuration)."""
    from mod_extraction_amd import models as amodels
    torch.manual_seed(0)
    model = amodels.SpectralTCN(n_samples=22272, out_channels=[16, 16], dilations=[1, 2]).to(dev).train()
    x = _dv(dev, _audio(2, 22272, 5, ch=1))

    def case():
        model.zero_grad(set_to_none=True)
        y = model(x)
        wy = torch.linspace(0.5, 1.5, y.numel(), device=dev).view_as(y)
        (y * wy).sum().backward()
        res = {"y": y}
        res.update({"grad/" + n: p.grad for n, p in model.named_parameters()})
        return res

    run_patterns(case, {"models:log_power", "tcn:forward", "tcn:backward"})


def test_generic_lstm(dev):
    """tests/test_gpu_generic_lstm.py's smallest size (1, 1, 7, 1), two chunks: the second starts from a carried state."""
    from mod_extraction_amd import models as amodels
    torch.manual_seed(0)
    model = amodels.LSTMEffectModel(1, 1, 7, 1)
    assert model.generic
    model = model.to(dev)
    B, Tn = 3, 300
    r = _rng(6)
    xs = [_dv(dev, r.random((B, 1, Tn)) * 1.6 - 0.8) for _ in range(2)]
    lats = [_dv(dev, r.random((B, 1, Tn))) for _ in range(2)]
    ws = [_dv(dev, r.random((B, 1, Tn)) - 0.5) for _ in range(2)]

    def case():
        model.clear_hidden()
        res = {}
        for c in range(2):
            model.zero_grad(set_to_none=True)
            lat = lats[c].clone().requires_grad_(True)
            y = model(xs[c], lat)
            (y * ws[c]).sum().backward()
            res.update({f"y{c}": y, f"dlat{c}": lat.grad, f"h{c}": model.hidden[0], f"c{c}": model.hidden[1]})
            res.update({f"grad{c}/" + n: p.grad for n, p in model.named_parameters()})
            model.detach_hidden()
        return res

    run_patterns(case, {"lstm_generic:_empty"})


# ---------------------------------------------------------------------------------------------------------------------
# LSTM effect model (the fused LSTM-64 kernels)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Tn", [(2, 300), (1, 1025)])
def test_lstm_effect_model(dev, B, Tn):
    from mod_extraction_amd import models as amodels
    torch.manual_seed(100 * B + Tn)
    model = amodels.LSTMEffectModel(1, 1, 64, 1).to(dev)
    assert not model.generic
    W = 40                                               # warm-up chunk: a non-zero state enters the chunk under test
    r = _rng(Tn)
    x = r.random((B, 1, W + Tn)) * 1.6 - 0.8
    wet = np.clip(0.6 * x + 0.3 * np.roll(x, 2, -1), -1, 1)
    xd, ld, wd = _dv(dev, x), _dv(dev, r.random((B, 1, W + Tn))), _dv(dev, wet)
    dyd = _dv(dev, r.standard_normal((B, 1, Tn)) / (B * Tn))
    xc, lc, wc = xd[..., W:], ld[..., W:], wd[..., W:]
    NP = amodels.LSTM_NPARAM

    def case():
        model.clear_hidden()
        y_w, _, _ = model.run_chunk(xd[..., :W], ld[..., :W])
        model.detach_hidden()
        stash = torch.empty((B, Tn, 384), device=dev)
        y, h0, c0 = model.run_chunk(xc, lc, stash)
        res = {"y_warm": y_w, "y": y, "h1": model.hidden[0], "c1": model.hidden[1]}
        res["l1_rows"] = model.bptt_l1_chunk(xc, lc, y, wc, stash, h0, c0, 1.0 / (B * Tn), None)
        g = [torch.empty(NP, device=dev) for _ in range(4)]
        model.bptt_l1_chunk(xc, lc, y, wc, stash, h0, c0, 1.0 / (B * Tn), g[0])
        model.bptt_chunk(xc, lc, y, dyd, stash, h0, c0, g[1])
        res["dlfo_l1"] = model.bptt_chunk_dlfo(xc, lc, y, stash, h0, c0, g[2], wet=wc, loss_scale=1.0 / (B * Tn))
        res["dlfo_dy"] = model.bptt_chunk_dlfo(xc, lc, y, stash, h0, c0, g[3], dy=dyd)
        res.update({"g_l1": g[0], "g_dy": g[1], "g_dlfo_l1": g[2], "g_dlfo_dy": g[3]})
        return res

    run_patterns(case, {"models:run_chunk", "models:bptt_l1_chunk", "models:bptt_chunk", "models:bptt_chunk_dlfo"})


# ---------------------------------------------------------------------------------------------------------------------
# effects
# ---------------------------------------------------------------------------------------------------------------------
def _fx_cases():
    """(B, N, n_mod, rows): full-rate and low-rate LFO at both shapes, and the rows subset [0, 2] at B = 3."""
    return [(3, 1000, 1000, None), (3, 1000, 87, None), (1, 4099, 4099, None), (1, 4099, 345, None),
            (3, 1000, 1000, (0, 2)), (3, 1000, 87, (0, 2))]


FX_IDS = ["B3-N1000-full", "B3-N1000-lowrate", "B1-N4099-full", "B1-N4099-lowrate", "B3-N1000-full-rows", "B3-N1000-lowrate-rows"]


def _rows_t(dev, rows):
    return None if rows is None else torch.tensor(rows, dtype=torch.int32).to(dev)


def _filled(dev, shape, dtype=torch.float32):
    """A caller's own output buffer with known content (made through torch.full: not a poisoned allocation)."""
    return torch.full(shape, 7.0, dtype=dtype).to(dev)


@pytest.mark.parametrize("B,N,n_mod,rows", _fx_cases(), ids=FX_IDS)
def test_flanger(dev, B, N, n_mod, rows):
    """flanger_forward, flanger_forward_stash and flanger_backward (mx_flanger_bwd at n_mod == N, mx_flanger_bwd_lr below).
    With a rows subset the outputs are the caller's own buffers: the rows that are not listed keep what they held."""
    from mod_extraction_amd import fx
    M = 100
    r = _rng(N + n_mod)
    consts = fx.derive_clip_constants(B, dev, 40, 60, _dv("cpu", 0.2 + 0.5 * r.random(B)), 0.5, 1.0,
                                      _dv("cpu", 0.5 + 0.4 * r.random(B)), _dv("cpu", 0.3 + 0.5 * r.random(B)), check=False)
    md = torch.full((B,), M, dtype=torch.int32).to(dev)
    x, mod, dy = _dv(dev, _audio(B, N, 7)), _dv(dev, _lfo_rows(B, n_mod, 8)), _dv(dev, r.standard_normal((B, N)))
    rt = _rows_t(dev, rows)

    def case():
        own = rows is not None
        y_plain = fx.flanger_forward(x, mod, consts, md, M, rows=rt, out=_filled(dev, (B, N)) if own else None)
        y, st = fx.flanger_forward_stash(x, mod, consts, md, M, rows=rt, out=_filled(dev, (B, N)) if own else None,
                                         stash=_filled(dev, (B, N)) if own else None)
        dx, dmod, g = fx.flanger_backward(dy, x, mod, st, consts, md, M, rows=rt, dx=_filled(dev, (B, N)) if own else None,
                                          dmod=_filled(dev, (B, n_mod)) if own else None)
        res = {"y_plain": y_plain, "y": y, "stash": st, "dx": dx, "dmod": dmod}
        res.update({"g/" + k: v for k, v in g.items()})
        return res

    run_patterns(case, {"fx:flanger_backward"} | (set() if rows is not None else {"fx:flanger_forward", "fx:flanger_forward_stash"}))


def _phaser_params(dev, B, seed):
    r = _rng(seed)
    return {"rate_hz": _dv(dev, 0.5 + 2.5 * r.random(B)), "depth": _dv(dev, 0.4 + 0.5 * r.random(B)),
            "centre_frequency_hz": _dv(dev, 400.0 + 2000.0 * r.random(B)), "feedback": _dv(dev, -0.5 + r.random(B)),
            "mix": _dv(dev, 0.3 + 0.5 * r.random(B))}


@pytest.mark.parametrize("B,N,n_mod,rows", _fx_cases(), ids=FX_IDS)
def test_phaser(dev, B, N, n_mod, rows):
    """phaser_forward (built-in oscillator); at n_mod == N the external LFO at the cut-off-update rate (one value per 4
    samples: phaser_forward_stash / phaser_backward), below it the low-rate path (phaser_forward_stash_lr / phaser_backward_lr
    = phaser_mod_expand + stash forward, backward + phaser_dmod_gather)."""
    from mod_extraction_amd import fx
    params = _phaser_params(dev, B, N + n_mod)
    src, dy = _dv(dev, _audio(B, N, 9)), _dv(dev, _rng(10).standard_normal((B, N)))
    ng = (N + 3) // 4
    low_rate = n_mod != N
    mod = _dv(dev, _lfo_rows(B, n_mod if low_rate else ng, 11))
    rt = _rows_t(dev, rows)
    own = rows is not None
    listed = list(rows) if own else slice(None)
    _, stash_row = fx.phaser_stash_shape(N)

    def case():
        res = {"y_osc": fx.phaser_forward(src, params, None, SR, N, rows=rt, out=_filled(dev, (B, N)) if own else None)}
        out = _filled(dev, (B, N)) if own else None
        if low_rate:
            y, st, mod_g = fx.phaser_forward_stash_lr(src, params, None, SR, N, mod, rows=rt, out=out)
            dx, dmod, g = fx.phaser_backward_lr(dy, src, st, params, None, SR, N, n_mod, rows=rt,
                                                dmod=_filled(dev, (B, n_mod)) if own else None)
            # fx.phaser_forward_stash_lr: "the other rows of ``out`` ... are not touched, those of stash and mod_g are
            # uninitialised"; fx.phaser_backward_lr: "dmod: an optional (B, n_mod) dense output whose listed rows are written and
            # whose other rows are not touched (without it they are uninitialised, as are those of dx)"
            res.update({"mod_g": mod_g[listed], "stash": st[listed], "dx": dx[listed]})
        else:
            y, st = fx.phaser_forward_stash(src, params, None, SR, N, mod=mod, rows=rt, out=out,
                                            stash=_filled(dev, (B, stash_row)) if own else None)
            dx, dmod, g = fx.phaser_backward(dy, src, st, params, None, SR, N, rows=rt, dx=_filled(dev, (B, N)) if own else None,
                                             dmod=_filled(dev, (B, ng)) if own else None)
            res.update({"stash": st, "dx": dx})
        res.update({"y": y, "dmod": dmod})
        res.update({"g/" + k: v for k, v in g.items()})
        return res

    expect = {"fx:phaser_forward"}                          # its cut-off workspace, with and without rows
    if low_rate:
        expect |= {"fx:phaser_mod_expand", "fx:phaser_forward_stash", "fx:phaser_backward"}
    elif not own:
        expect |= {"fx:phaser_forward_stash", "fx:phaser_backward"}
    run_patterns(case, expect)


@pytest.mark.parametrize("B,N,n_mod,rows", _fx_cases(), ids=FX_IDS)
def test_phaser_mod_expand_and_dmod_gather(dev, B, N, n_mod, rows):
    """The two launches on their own, with a per-clip lead-in in front of the clip window."""
    from mod_extraction_amd import fx
    if n_mod == N:
        n_mod = N // 4                                          # (a low-rate row by definition: the group rate is the upper end)
    lead_h = np.asarray([0, 37, 122][:B], np.int32)
    width = N + 128
    lead = torch.from_numpy(lead_h).to(dev)
    mod = _dv(dev, _lfo_rows(B, n_mod, 12))
    ng = (width + 3) // 4
    dmod_g = _dv(dev, _rng(13).standard_normal((B, ng)))
    rt = _rows_t(dev, rows)
    own = rows is not None

    def case():
        # with rows the outputs are the caller's buffers (fx.phaser_mod_expand / fx.phaser_dmod_gather: "the others of ``out``
        # are not touched (without ``out`` they are uninitialised)")
        mod_g = fx.phaser_mod_expand(mod, lead, N, width, rows=rt, out=_filled(dev, (B, ng)) if own else None)
        d_lr = fx.phaser_dmod_gather(dmod_g, lead, N, n_mod, rows=rt, out=_filled(dev, (B, n_mod)) if own else None)
        res = {"mod_g": mod_g, "dmod_lr": d_lr}
        if own:                                                 # ... and once without ``out``: the listed rows
            res["mod_g_listed"] = fx.phaser_mod_expand(mod, lead, N, width, rows=rt)[list(rows)]
            res["dmod_lr_listed"] = fx.phaser_dmod_gather(dmod_g, lead, N, n_mod, rows=rt)[list(rows)]
        return res

    run_patterns(case, {"fx:phaser_mod_expand", "fx:phaser_dmod_gather"})


@pytest.mark.parametrize("B,N,n_mod,rows", _fx_cases(), ids=FX_IDS)
def test_tremolo(dev, B, N, n_mod, rows):
    from mod_extraction_amd import fx
    r = _rng(N + n_mod + 1)
    consts = fx.derive_tremolo_constants(B, dev, _dv("cpu", 0.2 + 0.7 * r.random(B)), check=False)
    x, mod, dy = _dv(dev, _audio(B, N, 14)), _dv(dev, _lfo_rows(B, n_mod, 15)), _dv(dev, r.standard_normal((B, N)))
    rt = _rows_t(dev, rows)
    own = rows is not None

    def case():
        # fx.tremolo_forward: "rows: optional int32 list of the rows to process (the others of ``out`` are untouched)": with
        # rows the output is the caller's buffer.  fx.tremolo_backward: "rows not listed in ``rows`` hold zeros": compared whole.
        y = fx.tremolo_forward(x, mod, consts, rows=rt, out=_filled(dev, (B, N)) if own else None)
        dx, dmod, dmix = fx.tremolo_backward(dy, x, mod, consts, rows=rt)
        res = {"y": y, "dx": dx, "dmod": dmod, "dmix": dmix}
        if own:                                 # ... and once into a fresh output, whose other rows are what the allocation held
            res["y_listed"] = fx.tremolo_forward(x, mod, consts, rows=rt)[list(rows)]
        return res

    # (with rows every output of tremolo_backward comes from torch.zeros: test_sensitivity_control_... is about that branch)
    run_patterns(case, {"fx:tremolo_forward"} | (set() if own else {"fx:tremolo_backward"}))


def test_sensitivity_control_tremolo_backward_zero_fill(dev):
    """The probe sees a zero-fill that is needed: fx.tremolo_backward promises "rows not listed in ``rows`` hold zeros" and gets
    them from torch.zeros.  With torch.zeros poisoned as well, row 1 of dx holds the poison; with it left alone, zeros."""
    from mod_extraction_amd import fx
    B, N = 3, 1000
    consts = fx.derive_tremolo_constants(B, dev, 0.6, check=False)
    x, mod, dy = _dv(dev, _audio(B, N, 16)), _dv(dev, _lfo_rows(B, N, 17)), _dv(dev, _rng(18).standard_normal((B, N)))
    rt = _rows_t(dev, (0, 2))
    got = {}
    for pat in ("A", "B"):
        for also in (True, False):
            with poisoned(pat, also_zeros=also) as ctx:
                dx, _, _ = fx.tremolo_backward(dy, x, mod, consts, rows=rt, need_dx=True)
                torch.cuda.synchronize()
            got[pat, also] = dx.cpu()
            assert (ctx.sites[PKG + "fx:tremolo_backward"] >= 1) == also        # every allocation of this branch is a torch.zeros
    assert bool((got["B", True][1] == 0.5).all())
    assert bool((got["B", False][1] == 0.0).all())
    assert bool((got["A", True][1] == 0.0).all()) and bool((got["A", False][1] == 0.0).all())
    for key in (("A", False), ("B", True), ("B", False)):                      # the listed rows never depend on it
        assert torch.equal(got[key][[0, 2]], got["A", True][[0, 2]])
    assert bool((got["A", True][[0, 2]] != 0).any())


FX_SPEC = {"flanger": {"feedback": {"min": 0.1, "max": 0.9, "init": 0.5}, "width": {"min": 0.2, "max": 1.0, "init": 0.6},
                       "min_delay_width": 0.4, "mix": {"min": 0.1, "max": 1.0, "init": 0.7}},
           "phaser": {"centre_frequency_hz": {"min": 200.0, "max": 4000.0, "init": 1000.0},
                      "depth": {"min": 0.1, "max": 1.0, "init": 0.5}},
           "tremolo": {"mix": {"min": 0.2, "max": 1.0, "init": 0.5}}}


def _fx_rows(dev, B, seed):
    from mod_extraction_amd import fx
    r = _rng(seed)
    kinds = [fx.FX_KINDS.index(k) for k in ("flanger", "phaser", "tremolo")][:B]
    row_kind = torch.tensor(kinds, dtype=torch.int32).to(dev)
    consts0 = {k: _dv(dev, 0.1 + 0.8 * r.random(B)) for k in fx.FX_CONSTS}
    grads = _dv(dev, r.standard_normal((len(fx.FX_SLOTS), B)), np.float64)
    return row_kind, consts0, _dv(dev, np.full(B, 60.0)), _dv(dev, np.full(B, 40.0)), grads


@pytest.mark.parametrize("B", [3, 1])
def test_fx_params_expand_and_grad(dev, B):
    from mod_extraction_amd import fx
    table = fx.LearnedFxParams(FX_SPEC, raw_gain=2.0)
    with torch.no_grad():
        table.raw.add_(torch.linspace(-0.4, 0.5, table.raw.numel()))
    table = table.to(dev)
    row_kind, consts0, max_lfo, max_min, grads = _fx_rows(dev, B, 19)

    def case():
        consts = {k: v.clone() for k, v in consts0.items()}
        values = table.expand(consts, row_kind, max_lfo, max_min)
        d_raw = table.grad(grads, row_kind, max_lfo, max_min, scale=0.5)
        res = {"values": values, "d_raw": d_raw}
        res.update({"consts/" + k: v for k, v in consts.items()})
        return res

    run_patterns(case, {"fx:fx_params_expand", "fx:fx_params_grad"})


@pytest.mark.parametrize("B", [3, 1])
def test_fx_head_forward_and_backward(dev, B):
    from mod_extraction_amd import fx
    C, W = 64, 88
    head = fx.FxParamHead(FX_SPEC, in_ch=C, raw_gain=2.0)
    with torch.no_grad():
        head.weight.copy_(torch.from_numpy(_rng(20).standard_normal(tuple(head.weight.shape)).astype(np.float32)) * 0.1)
    head = head.to(dev)
    row_kind, consts0, max_lfo, max_min, grads = _fx_rows(dev, B, 21)
    latent = _dv(dev, _rng(22).standard_normal((B, C, W)))

    def case():
        consts = {k: v.clone() for k, v in consts0.items()}
        pooled, raw_rows, values = head.forward_rows(latent, consts, row_kind, max_lfo, max_min)
        d_rows, d_bias, d_weight, d_latent = fx.fx_head_backward(grads, raw_rows, pooled, head.weight.detach(), head.tab_f,
                                                                 head.tab_i, head.raw_gain, row_kind, max_lfo, max_min, W,
                                                                 scale=0.5, need_d_raw_rows=True)
        res = {"pooled": pooled, "raw_rows": raw_rows, "values": values, "d_rows": d_rows, "d_bias": d_bias,
               "d_weight": d_weight, "d_latent": d_latent}
        res.update({"consts/" + k: v for k, v in consts.items()})
        return res

    run_patterns(case, {"fx:fx_head_forward", "fx:fx_head_backward"})


# ---------------------------------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------------------------------
def _loss_pair(dev, B, Tn, seed):
    a = _audio(B, Tn, seed)
    t = np.clip(0.7 * a + 0.25 * np.roll(a, 5, -1) + 0.02 * _rng(seed + 1).standard_normal((B, Tn)), -1, 1)
    return _dv(dev, a), _dv(dev, t)


@pytest.mark.parametrize("Tn", [4097, 9001])
def test_mrstft_loss(dev, Tn):
    from mod_extraction_amd import mrstft
    B = 2
    a, t = _loss_pair(dev, B, Tn, 23)
    mod = mrstft.MultiResolutionSTFTLoss()

    def case():
        value, dx = mrstft.mrstft_value_and_grad(mod, a, t, scale=0.75)
        terms = mod.last_terms
        v_only, none = mrstft.mrstft_value_and_grad(mod, a, t, need_grad=False)
        assert none is None
        y_hat = a.view(B, 1, Tn).clone().requires_grad_(True)
        loss = mod(y_hat, t.view(B, 1, Tn))
        (2.0 * loss).backward()
        return {"value": value, "dx": dx, "terms": terms, "value_only": v_only, "module_loss": loss, "module_grad": y_hat.grad}

    run_patterns(case, {"mrstft:mrstft_value_and_grad"})


@pytest.mark.parametrize("Tn", [4097, 9001])
def test_logmel_l1_and_pre_emph_esr_losses(dev, Tn):
    from mod_extraction_amd import losses
    B = 2
    a, t = _loss_pair(dev, B, Tn, 24)
    logmel = losses.LogMelLoss()
    esr_pre = losses.PreEmphESRLoss(filter_cfs=(-0.95, 1.0), low_pass=True)

    def case():
        v, dx = losses.logmel_l1_value_and_grad(logmel, a, t, scale=0.5)
        v0, _ = losses.logmel_l1_value_and_grad(logmel, a, t, need_grad=False)
        vm = logmel(a.view(B, 1, Tn), t.view(B, 1, Tn))
        e, de = losses.pre_emph_esr_value_and_grad(esr_pre, a, t, scale=0.5)
        e0, _ = losses.pre_emph_esr_value_and_grad(esr_pre, a, t, need_grad=False)
        return {"logmel": v, "logmel_dx": dx, "logmel_value_only": v0, "logmel_module": vm, "esr_pre": e, "esr_pre_dx": de,
                "esr_pre_value_only": e0}

    run_patterns(case, {"losses:logmel_l1_value_and_grad", "losses:pre_emph_esr_value_and_grad"})


@pytest.mark.parametrize("Tn", [4097, 9001])
def test_effect_loss_terms_and_grad(dev, Tn):
    from mod_extraction_amd import effect_losses
    B = 2
    a, t = _loss_pair(dev, B, Tn, 25)
    y_hat, y = a.view(B, 1, Tn), t.view(B, 1, Tn)

    def case():
        res = {"term/" + k: v for k, v in effect_losses.effect_loss_terms(y_hat, y).items()}
        res["dy_plain"] = effect_losses.effect_loss_grad(y_hat, y, {"l1": 1.0, "mse": 0.5, "esr": 0.25, "dc": 0.125})
        values = {}
        res["dy_all"] = effect_losses.effect_loss_grad(y_hat, y, {"l1": 1.0, "esr": 0.25, "mrstft": 0.5, "log_mel_l1": 0.3,
                                                                  "esr_pre": 0.2}, values=values)
        res.update({"value/" + k: v for k, v in values.items()})
        return res

    run_patterns(case, {"effect_losses:effect_loss_terms", "effect_losses:effect_loss_grad", "mrstft:mrstft_value_and_grad",
                        "losses:logmel_l1_value_and_grad", "losses:pre_emph_esr_value_and_grad"})


@pytest.mark.parametrize("n", [5, 345])
def test_lfo_loss(dev, n):
    from mod_extraction_amd import losses
    r = _rng(n)
    yh0, y = _dv(dev, r.random((7, n))), _dv(dev, r.random((7, n)))
    w = {"l1": 1.0, "fdl1": 5.0, "sdl1": 10.0, "mse": 0.0}

    def case():
        yh = yh0.clone().requires_grad_(True)
        total, terms = losses.lfo_loss(yh, y, w)
        (3.0 * total).backward()
        res = {"total": total, "grad": yh.grad}
        res.update({"term/" + k: v for k, v in terms.items()})
        return res

    run_patterns(case, {"losses:forward"})


# ---------------------------------------------------------------------------------------------------------------------
# LFO ops
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 345])
@pytest.mark.parametrize("B", [4, 130])
def test_lfo_ops(dev, B, n):
    from mod_extraction_amd import modulations as M, util
    r = _rng(B + n)
    sr = n / 2.0                                              # the rows span 2 s
    f_hi = min(5.0, 0.4 * sr / 2.0)
    freq, phase = _dv(dev, 0.6 + (f_hi - 0.6) * r.random(B)), _dv(dev, 2 * np.pi * r.random(B))
    shape = torch.from_numpy(r.integers(0, 6, B).astype(np.int32)).to(dev)
    exp = _dv(dev, 0.5 + 2.0 * r.random(B))
    rows = _dv(dev, _lfo_rows(B, n, B + n + 1, hi=f_hi))
    S, k = 24, 4
    torch.manual_seed(B + n)
    shrink, amount = M.draw_quasi_tables(B, S)
    table = M.draw_combined_table(B, S, ["cos", "tri", "rect_cos", "inv_rect_cos", "saw", "rsaw"])
    shrink, amount, table = shrink.to(dev), amount.to(dev), table.to(dev)
    d_out = _dv(dev, r.standard_normal((B, n - k + 1)))
    n_other = 345 if n == 33 else 33
    dy_interp = _dv(dev, r.standard_normal((B, n_other - 4)))

    def case():
        res = {"synth": M.make_mod_signals(n, sr, freq, phase, shape, exp),
               "synth_resampled": M.make_mod_signals(4 * n, 4 * sr, freq, phase, shape, n_out=n)}
        res["quasi"], res["quasi_n_corners"] = M.make_quasi_periodic_batch(rows, shrink, amount)
        res["combined"], res["combined_n_corners"] = M.make_combined_mod_sigs(n, sr, freq, phase, table)
        res["smooth"] = M.smoothen(rows, k)
        res["top"], res["bottom"] = M.find_corners(rows)
        res["stretched"] = M.stretch_corners(rows, max_n_corners=16, smooth_n_frames=k)
        res["stretched_bwd"] = M.stretch_corners_bwd(rows, d_out, max_n_corners=16, smooth_n_frames=k)
        res["valid"] = M.valid_mod_sig_mask(rows)
        fit = M.fit_lfo(rows, sr, rate_hz=(0.25, min(8.0, 0.45 * sr)), per_shape=True)
        res.update({"fit/" + name: getattr(fit, name) for name in fit._fields})
        res["interp"] = util.linear_interpolate_last_dim(rows, n_other)
        res["interp_bwd"] = util.linear_interpolate_last_dim_bwd(dy_interp, n, n_other, j0=2)
        return res

    run_patterns(case, {"modulations:make_mod_signals", "modulations:make_quasi_periodic_batch", "modulations:make_combined_mod_sigs",
                        "modulations:smoothen", "modulations:find_corners", "modulations:stretch_corners",
                        "modulations:stretch_corners_bwd", "modulations:valid_mod_sig_mask", "modulations:fit_lfo",
                        "util:linear_interpolate_last_dim", "util:linear_interpolate_last_dim_bwd"})


# ---------------------------------------------------------------------------------------------------------------------
# pair utilities
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L", [(257, 16), (4099, 64)])
def test_pair_alignment(dev, N, L):
    from mod_extraction_amd import alignment as A
    B = 3
    dry = _audio(B, N, N)
    wet = np.stack([np.roll(dry[0], 5), -np.roll(dry[1], -3), 0.5 * dry[2]]).astype(np.float32)
    d, w = _dv(dev, dry), _dv(dev, wet)
    lag_in = torch.tensor([5, -3, 0], dtype=torch.int32).to(dev)
    corr_in = torch.tensor([0.9, -0.8, 0.5], dtype=torch.float32).to(dev)

    def case():
        est = A.estimate_pair_lag(d, w, L)
        res = {"xcorr": A.xcorr_lags(d, w, L), "lag": est.lag, "frac": est.frac, "corr": est.corr}
        res["shifted"] = A.shift_rows(w, lag_in, corr_in)
        res["shifted_plain"] = A.shift_rows(w.view(B, 1, N), lag_in)
        res["aligned"], _ = A.align_pairs(d, w, L)
        return res

    run_patterns(case, {"alignment:_xcorr", "alignment:estimate_pair_lag", "alignment:shift_rows"})


@pytest.mark.parametrize("mode", ["ls", "rms"])
@pytest.mark.parametrize("N", [5, 2051])                        # gain.CHUNK + 3: two workgroups a row
def test_gain_match(dev, N, mode):
    from mod_extraction_amd import gain as G
    B = 3
    r = _rng(N)
    p = r.standard_normal((B, N))
    q = np.asarray([[0.5], [2.0], [40.0]]) * (p + 0.05 * r.standard_normal((B, N)))
    y_hat, y, dz = _dv(dev, p), _dv(dev, q), _dv(dev, r.standard_normal((B, N)))

    def case():
        res = {}
        for name, rng in (("free", None), ("clamped", (0.25, 4.0))):
            m = G.match_gain(y_hat, y, mode, gain_range=rng)
            d = G.match_gain_backward(dz, y_hat, y, m, mode)
            res.update({f"{name}/z": m.z, f"{name}/gain": m.gain, f"{name}/sums": m.sums, f"{name}/flags": m.flags,
                        f"{name}/dy_hat": d})
        return res

    run_patterns(case, {"gain:match_gain", "gain:match_gain_backward"})


@pytest.mark.parametrize("low_pass", [False, True])
def test_pre_emph_rows(dev, low_pass):
    from mod_extraction_amd import wright_code as W
    taps = W.PreEmphTaps((-0.95, 1.0), low_pass)
    res_in = {}
    for B, n in ((3, 257), (1, 4099)):
        res_in[B, n] = (_dv(dev, _audio(B, n, n)), _dv(dev, _rng(n).standard_normal((B, taps.out_len(n)))))

    def case():
        res = {}
        for (B, n), (x, g) in res_in.items():
            res[f"fwd/{B}x{n}"] = W.pre_emph_rows(taps, x)
            res[f"bwd/{B}x{n}"] = W.pre_emph_rows(taps, g, transpose=True, n=n)
            a, t = x.t().unsqueeze(-1), (0.8 * x).roll(3, -1).t().unsqueeze(-1)          # time-major (T, B, 1)
            res[f"wright_esr/{B}x{n}"], res[f"wright_dc/{B}x{n}"] = W.WrightESRLoss()(a, t), W.WrightDCLoss()(a, t)
        return res

    run_patterns(case, {"wright_code:pre_emph_rows", "wright_code:_global_sums"})


# ---------------------------------------------------------------------------------------------------------------------
# whole steps
# ---------------------------------------------------------------------------------------------------------------------
def test_mixed_effect_audio_loss_step_with_learned_parameters(dev):
    """lightning.LFOExtractionThroughEffect on a batch that mixes all five kinds, with learned effect parameters: every family
    renders its listed rows into ONE wet_hat from torch.empty, the adjoints write their rows of one gradient and of the (6, B)
    parameter gradients ("rows of kinds without an entry for a slot are not read and may be uninitialised",
    fx.fx_params_grad).  The shapes of tests/test_gpu_learned_fx_step.py::test_parameter_gradient_against_fp64."""
    from mod_extraction_amd import fx, lightning
    kinds = ("flanger", "chorus", "phaser", "tremolo", "dry")
    unit = {"min": 0.0, "max": 1.0, "init": 0.5}
    delay = {"feedback": {"min": 0.0, "max": 0.7, "init": 0.3}, "min_delay_width": unit, "width": unit, "depth": unit, "mix": unit}
    spec = {"flanger": delay, "chorus": delay, "tremolo": {"mix": unit},
            "phaser": {"depth": {"min": 0.2, "max": 1.0, "init": 0.6}, "feedback": {"min": -0.7, "max": 0.7, "init": 0.2},
                       "centre_frequency_hz": {"min": 200.0, "max": 4000.0, "init": 1000.0}, "mix": unit}}
    B, N, n_mod = 5, 4096, 17
    r = _rng(44)
    dry, wet = _dv(dev, 0.3 * r.standard_normal((B, 1, N))), _dv(dev, 0.3 * r.standard_normal((B, 1, N)))
    step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=44100, effect=kinds,
                                                audio_loss_dict={"mrstft": 1.0, "l1": 0.5, "esr_pre": 0.25},
                                                learned_fx=fx.LearnedFxParams(spec, raw_gain=2.0))
    with torch.no_grad():
        step.learned_fx.raw.copy_(torch.from_numpy(r.uniform(-0.75, 0.75, step.learned_fx.raw.numel()).astype(np.float32)))
    step = step.to(dev)
    h0 = _dv(dev, _lfo_rows(B, n_mod, 45, lo=0.5, hi=1.25))

    def case():
        step.zero_grad(set_to_none=True)
        h = h0.clone().requires_grad_(True)
        loss, wet_hat = step.audio_loss(h, dry, wet, None)
        loss.backward()
        return {"loss": loss, "wet_hat": wet_hat, "dmod": h.grad, "d_raw": step.learned_fx.raw.grad}

    run_patterns(case, {"lightning:forward", "lightning:_render_rows", "fx:fx_params_expand", "fx:fx_params_grad",
                        "fx:flanger_backward", "fx:phaser_backward", "mrstft:mrstft_value_and_grad"})



def test_whole_lfo_extraction_step(dev):
    """Batch synthesis -> log-mel -> CNN -> LFO loss -> backward into the flat gradient buffer, with the batcher and the
    optimizer built inside the context: their own torch.empty buffers are poisoned before first use."""
    from mod_extraction_amd import data_modules, lightning, models as amodels, optim
    n, sr, B = 22272, 44100, 4
    cfg = dict(in_ch=2, n_samples=n, sr=sr, n_fft=1024, hop_len=256, n_mels=64, kernel_size=(5, 13), out_channels=[64] * 6,
               temp_dilations=[1, 1, 2, 4, 8, 16], pool_size=(2, 1), latent_dim=1, use_ln=True)
    ld = {"l1": 1.0, "fdl1": 5.0, "sdl1": 10.0, "mse": 0.0}              # tests/test_gpu_edges.py::test_lfo_extraction_sub_batch_size_path
    torch.manual_seed(21)
    state = amodels.Spectral2DCNN(**cfg).state_dict()

    def case():
        torch.manual_seed(5)
        np.random.seed(5)
        model = amodels.Spectral2DCNN(**cfg)
        model.load_state_dict(state)
        module = lightning.LFOExtraction(model, sr=sr, use_dry=True, model_smooth_n_frames=0, should_stretch=False,
                                         sub_batch_size=None, loss_dict=ld).to(dev).eval()
        opt = optim.FlatAdamW(module.parameters(), lr=1e-4, betas=(0.8, 0.99))
        batcher = data_modules.SyntheticFxBatcher(B, n, sr, ("flanger", "chorus", "phaser"), dev, audio_seed=1)
        dry, wet, mod, _ = batcher.render(batcher.sample_params())
        opt.zero_grad()
        loss = module.training_step((dry, wet, mod, None), 0)
        with opt.direct_backward():
            loss.backward()
        return {"dry": dry, "wet": wet, "mod": mod, "loss": loss, "flat_grad": opt.flat_grad, "flat_param": opt.flat_param}

    run_patterns(case, CNN_SITES_F16 | {"optim:__init__", "data_modules:__init__", "losses:forward",
                                        "util:linear_interpolate_last_dim"}, forbid={FRESH_GRADS})

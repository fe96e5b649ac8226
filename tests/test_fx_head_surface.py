"""CPU: the surface of the per-clip effect-parameter head -- ``fx.FxParamHead``'s construction (the spec grammar and errors
of ``fx.LearnedFxParams``), its parameters and state dict, ``LFOExtractionThroughEffect(fx_head=...)``'s errors, the two C-ABI
entry points, the shipped config, and the numpy fp64 restatement tests/helpers/fx_head64.py against ``FxParamHead.values``
and against central finite differences.  No device work."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests.helpers import fx_head64 as hh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
OK = {"min": 0.0, "max": 0.9, "init": 0.3}
FIVE = ("flanger", "chorus", "phaser", "tremolo", "dry")
UNIT = {"min": 0.0, "max": 1.0, "init": 0.5}
DELAY = {"feedback": {"min": 0.0, "max": 0.95, "init": 0.3}, "min_delay_width": UNIT, "width": UNIT, "depth": UNIT, "mix": UNIT}
SPEC15 = {"flanger": DELAY, "chorus": DELAY, "tremolo": {"mix": UNIT},
          "phaser": {"depth": {"min": 0.05, "max": 1.0, "init": 0.5, "scale": "log"}, "feedback": {"min": -0.9, "max": 0.9, "init": 0.1},
                     "centre_frequency_hz": {"min": 200.0, "max": 4000.0, "init": 1000.0}, "mix": UNIT}}

BAD_SPECS = [
    {"wah": {"mix": OK}}, {"dry": {"mix": OK}}, {"tremolo": {"depth": OK}}, {"flanger": {"rate_hz": OK}},
    {"flanger": {"depth": {"min": 0.0, "max": 1.0, "init": 0.0}}}, {"flanger": {"depth": {"min": 0.6, "max": 0.4, "init": 0.5}}},
    {"flanger": {"depth": {"min": 0.0, "max": 1.0}}}, {"flanger": {"feedback": {"min": 0.0, "max": 1.0, "init": 0.5}}},
    {"phaser": {"feedback": {"min": -1.0, "max": 0.9, "init": 0.0}}},
    {"phaser": {"centre_frequency_hz": {"min": 0.0, "max": 4000.0, "init": 1000.0}}},
    {"phaser": {"depth": {"min": 0.1, "max": 1.0, "init": 0.5, "scale": "cubic"}}}, {"tremolo": {"mix": 1.5}},
    {"flanger": {"width": 0.5}}, {}, {"flanger": 3.0},
]


@pytest.mark.parametrize("spec", BAD_SPECS)
def test_spec_errors_are_those_of_learned_fx(spec):
    """One parser: the same specs are refused, with the same message but for the argument's name."""
    from mod_extraction_amd import fx
    with pytest.raises(ValueError) as a:
        fx.LearnedFxParams(spec)
    with pytest.raises(ValueError) as b:
        fx.FxParamHead(spec, in_ch=3)
    assert str(b.value) == str(a.value).replace("learned_fx", "fx_head")


def test_names_parameters_and_state_dict():
    from mod_extraction_amd import fx
    spec = {"phaser": {"mix": OK, "depth": OK}, "flanger": {"mix": OK, "feedback": OK, "width": 0.5}, "tremolo": {"mix": OK}}
    head, lf = fx.FxParamHead(spec, in_ch=5, raw_gain=2.0), fx.LearnedFxParams(spec, raw_gain=2.0)
    assert head.names == lf.names == ["phaser.depth", "phaser.mix", "flanger.feedback", "flanger.mix", "tremolo.mix"]
    assert head.kinds == lf.kinds and head.fixed == lf.fixed == {("flanger", "width"): 0.5}
    assert torch.equal(head.tab_f, lf.tab_f) and torch.equal(head.tab_i, lf.tab_i) and head.raw_gain == 2.0
    assert head.learned("flanger") == ("feedback", "mix") and head.covers("flanger", "width") and not head.covers("flanger", "depth")
    assert head.weight.shape == (5, 5) and head.weight.dtype == torch.float32 and not bool(head.weight.any())
    assert torch.equal(head.bias.detach(), lf.raw.detach())                  # logit(init) / raw_gain: the very bits
    assert abs(float(head.bias.detach()[0]) - math.log(1.0 / 2.0) / 2.0) < 1e-7       # init 0.3 of [0, 0.9]: s = 1 / 3
    assert [k for k, _ in head.named_parameters()] == ["weight", "bias"] and list(head.state_dict()) == ["weight", "bias"]
    assert fx.FxParamHead(spec).in_ch == 64
    # a fresh head is LearnedFxParams at its init, whatever the latent
    v = head.values(torch.randn(4, 5, 7))
    assert v.shape == (4, 5) and v.dtype == torch.float64 and torch.equal(v, lf.values().expand(4, 5))
    for bad in (0, -3, 1025, 2.5):
        with pytest.raises(ValueError):
            fx.FxParamHead(spec, in_ch=bad)
    with pytest.raises(ValueError):
        fx.FxParamHead(spec, in_ch=5, raw_gain=0.0)


class Stub(torch.nn.Module):
    """A model that returns what it is given (a tensor, or the (lfo, latent) pair), with one parameter of its own."""

    def __init__(self, out):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.out = out

    def forward(self, x):
        return self.out


def step_of(effect, model=None, **kw):
    from mod_extraction_amd import lightning
    return lightning.LFOExtractionThroughEffect(torch.nn.Linear(3, 2) if model is None else model, effect=effect, **kw)


def test_step_parameters_metrics_and_errors():
    from mod_extraction_amd import fx, trainer
    spec = {"flanger": {"feedback": OK, "depth": OK, "mix": 1.0, "width": 1.0, "min_delay_width": 0.5}}
    step = step_of("flanger", fx_head=dict(spec, in_ch=3))
    assert isinstance(step.fx_head, fx.FxParamHead) and step.learned_fx is None and step.fx_head.in_ch == 3
    assert [k for k, _ in step.named_parameters()] == ["model.weight", "model.bias", "fx_head.weight", "fx_head.bias"]
    assert list(step.state_dict()) == ["model.weight", "model.bias", "fx_head.weight", "fx_head.bias"]
    names = ["fx/flanger.feedback", "fx/flanger.depth", "fx_std/flanger.feedback", "fx_std/flanger.depth"]
    assert step.step_metric_names == names
    assert trainer.metric_names(step, "train") == ["train/mrstft", "train/loss"] + names
    assert trainer.metric_names(step, "val") == ["val/mrstft", "val/loss"]
    assert step.missing_fx_params(None, 8) == []
    module = fx.FxParamHead(spec, in_ch=3, raw_gain=2.0)
    assert step_of("flanger", fx_head=module).fx_head is module              # a module is taken as it is
    plain = step_of("flanger")                                               # without the argument nothing changes
    assert plain.fx_head is None and plain.step_metric_names == []
    assert list(plain.state_dict()) == ["model.weight", "model.bias"]
    with pytest.raises(ValueError, match="mutually exclusive"):
        step_of("flanger", fx_head=spec, learned_fx=spec)
    with pytest.raises(ValueError):
        step_of("tremolo", fx_head=spec)                                     # a kind the step does not have
    with pytest.raises(ValueError):
        step_of("flanger", fx_head=fx.LearnedFxParams(spec))                 # not a head
    short = {"flanger": {k: v for k, v in spec["flanger"].items() if k != "width"}}
    bad = step_of("flanger", fx_head=dict(short, in_ch=3))
    assert bad.missing_fx_params(None, 4) == ["flanger.width"] and bad.missing_fx_params({"width": 1.0}, 4) == []
    dry = torch.zeros(4, 1, 64)
    with pytest.raises(ValueError, match="flanger.width"):
        bad.common_step((dry, dry, None, None), is_training=True)


def test_model_without_a_latent_or_with_other_channels():
    spec = {"flanger": {"feedback": OK, "depth": OK, "mix": 1.0, "width": 1.0, "min_delay_width": 0.5}, "in_ch": 3}
    dry = torch.zeros(4, 1, 64)
    lfo = torch.zeros(4, 1, 8)
    with pytest.raises(ValueError, match="latent"):
        step_of("flanger", Stub(lfo), fx_head=spec).common_step((dry, dry, None, None), is_training=True)
    with pytest.raises(ValueError, match="latent"):
        step_of("flanger", Stub((lfo, None)), fx_head=spec).common_step((dry, dry, None, None), is_training=True)
    with pytest.raises(ValueError, match="5 channels"):
        step_of("flanger", Stub((lfo, torch.zeros(4, 5, 8))), fx_head=spec).common_step((dry, dry, None, None), is_training=True)
    step = step_of("flanger", Stub((lfo, torch.zeros(4, 3, 8))), fx_head=spec)
    with pytest.raises(ValueError, match="latent"):
        step.render(dry, lfo[:, 0], None)                                    # render needs the latent too
    with pytest.raises(ValueError, match="latent"):
        step.audio_loss(lfo[:, 0], dry, dry, None)
    from mod_extraction_amd import _hip
    with pytest.raises(_hip.HipLibraryError):                                # a good pair reaches the launch: no CPU fallback
        step.common_step((dry, dry, None, None), is_training=True)


def test_abi_has_the_two_entry_points():
    """The two entries are declared in include/modex_hip.h (section K17) like every other, and ``_hip.SIGNATURES``, the one
    binding table, is derived from that text (tests/test_abi.py holds the two to each other over all entry points)."""
    from mod_extraction_amd import _hip, build
    from tests.test_abi import header_arg_counts
    lib = ctypes.CDLL(build.build(verbose=False))
    counts = header_arg_counts()
    assert {n for n in counts if n.startswith("mx_fx_head_")} == {"mx_fx_head_fwd", "mx_fx_head_bwd"}
    for name, n in (("mx_fx_head_fwd", 24), ("mx_fx_head_bwd", 20)):
        assert hasattr(lib, name) and counts[name] == n == len(_hip.SIGNATURES[name]), name
    assert _hip.ABI_VERSION == 21 == lib.mx_abi_version()
    zeros = {ctypes.c_void_p: None, ctypes.c_int64: 0, ctypes.c_float: 0.0, ctypes.c_double: 0.0}
    for name in ("mx_fx_head_fwd", "mx_fx_head_bwd"):
        fn = getattr(_hip.load(), name)
        assert fn.argtypes == _hip.SIGNATURES[name]                          # load() binds the table
        assert fn(*[zeros[t] for t in fn.argtypes]) == -1, name
    # arguments are checked before any launch: P = 17, C = 1025 are refused without a device
    lib2 = _hip.load()
    one = ctypes.c_void_p(8)
    consts = (None,) * 7

    def fwd(B, C, W, P, pooled=one, lfo_scale=None):
        return lib2.mx_fx_head_fwd(one, B, C, W, one, one, one, one, P, 1.0, one, None, None, lfo_scale, *consts[1:], pooled, one,
                                   None, None)

    assert fwd(4, 64, 345, 17) == -2 and fwd(4, 1025, 345, 2) == -2 and fwd(4, 1024, 1 << 21, 2) == -2
    assert fwd(4, 64, 0, 2) == -1 and fwd(0, 64, 8, 2) == -1 and fwd(4, 64, 8, 2, pooled=None) == -1
    assert fwd(4, 64, 8, 2, lfo_scale=one) == -1                             # an lfo_scale output without its sample counts

    def bwd(B, C, W, P, counts_v=one):
        return lib2.mx_fx_head_bwd(one, one, one, one, one, one, P, 1.0, one, counts_v, counts_v, B, C, W, 1.0, None, one, one,
                                   one, None)

    assert bwd(4, 64, 345, 17) == -2 and bwd(4, 1025, 345, 2) == -2
    assert bwd(4, 64, 345, 2, counts_v=None) == -1 and bwd(4, 0, 345, 2) == -1


def table(mod):
    f, i = mod.tab_f.numpy(), mod.tab_i.numpy()
    return f[0], f[1], i[0], i[1], i[2]


def small_case(seed=17):
    """B = 5, one row per kind; C = 3; W = 7; the 15-entry table, raw_gain 1.5."""
    from mod_extraction_amd import fx
    head = fx.FxParamHead(SPEC15, in_ch=3, raw_gain=1.5)
    g = np.random.default_rng(seed)
    latent = g.normal(0.0, 1.0, (5, 3, 7))
    weight, bias = g.normal(0.0, 0.8, (15, 3)), g.uniform(-1.5, 1.5, 15)
    row_kind = np.arange(5, dtype=np.int32)
    ml = np.asarray([441.0, 441.0, 0.0, 0.0, 0.0])
    mm = np.asarray([44.0, 1323.0, 0.0, 0.0, 0.0])
    return head, latent, weight, bias, row_kind, ml, mm


def test_values_agree_with_the_helper():
    head, latent, weight, bias, *_ = small_case()
    lo, hi, is_log, _, _ = table(head)
    with torch.no_grad():
        head.weight.copy_(torch.tensor(weight))
        head.bias.copy_(torch.tensor(bias))
    # the module's parameters are fp32: the helper is fed what they hold
    w32, b32 = head.weight.detach().double().numpy(), head.bias.detach().double().numpy()
    lat = torch.tensor(latent)
    got = head.values(lat).detach().numpy()
    pooled, raw, want = hh.forward(latent, w32, b32, lo, hi, is_log, 1.5)
    assert got.shape == want.shape == (5, 15) and pooled.shape == (5, 3) and raw.shape == (5, 15)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"FxParamHead.values against the helper: max |difference| / max |value| {err:.3e}")
    assert err <= 1e-12
    assert float(np.abs(got[0] - got[1]).max()) > 1e-3                       # the rows differ: the weight is at work
    # differentiable with respect to the latent and both parameters
    lat.requires_grad_(True)
    head.values(lat).sum().backward()
    assert lat.grad is not None and head.weight.grad is not None and head.bias.grad is not None


def test_helper_backward_against_finite_differences():
    """L(weight, bias, pooled) = sum over the entries' own rows of scale * g[slot, b] * count * value(raw[b, e]) has
    d L / d raw = the helper's d_raw; its central differences (fp64, step 1e-5: truncation ~1e-10 relative) with respect to
    EVERY weight, bias and pooled element against the helper's d_weight, d_bias and d_pooled = W * d_latent.  Gate: worst
    |difference| <= 1e-6 of the largest magnitude of that gradient, the gate of the project's other finite-difference tests."""
    head, latent, weight, bias, row_kind, ml, mm = small_case()
    lo, hi, is_log, slot, kind = table(head)
    W, scale, gain = latent.shape[-1], 0.75, 1.5
    g = np.random.default_rng(3)
    grads = g.choice([-1.0, 1.0], (6, 5)) * 10.0 ** g.uniform(-1.0, 1.0, (6, 5))
    covered = np.zeros((6, 5), dtype=bool)
    for e in range(15):
        covered[slot[e]] |= row_kind == kind[e]
    poisoned = np.where(covered, grads, np.nan)                              # what no entry covers is never read
    pooled, _ = hh.pool(latent)

    def L(weight, bias, pooled):
        raw, _ = hh.linear(pooled, weight, bias)
        v = hh.values(raw, lo, hi, is_log, gain)
        total = 0.0
        for e in range(15):
            for b in np.nonzero(row_kind == kind[e])[0]:
                count = ml[b] if hh.SLOTS[slot[e]] == "lfo_scale" else mm[b] if hh.SLOTS[slot[e]] == "min_delay" else 1.0
                total += scale * grads[slot[e], b] * count * v[b, e]
        return total

    raw, _ = hh.linear(pooled, weight, bias)
    out = hh.backward(poisoned, raw, pooled, weight, lo, hi, is_log, slot, kind, gain, row_kind, ml, mm, W, scale)
    assert all(np.isfinite(out[k]).all() for k in out)
    assert not out["d_raw"][4].any() and not out["d_latent"][4].any()        # the dry row
    assert np.allclose(out["d_latent"] * W, out["d_pooled"], rtol=1e-15, atol=0.0)
    step = 1e-5
    args = {"d_weight": weight, "d_bias": bias, "d_pooled": pooled}
    for pos, key in enumerate(("d_weight", "d_bias", "d_pooled")):
        base = args[key]
        fd = np.zeros_like(base)
        for idx in np.ndindex(*base.shape):
            up, dn = base.copy(), base.copy()
            up[idx] += step
            dn[idx] -= step
            a = [weight, bias, pooled]
            a[pos] = up
            f_up = L(*a)
            a[pos] = dn
            fd[idx] = (f_up - L(*a)) / (2.0 * step)
        worst = float(np.abs(fd - out[key]).max() / np.abs(out[key]).max())
        print(f"{key}: {base.size} elements, worst |finite difference - helper| / max |helper| {worst:.3e}")
        assert worst <= 1e-6, key


def test_shipped_config_and_state_dict():
    from mod_extraction_amd import cli, data_modules, fx, lightning, models

    def build():
        old = os.getcwd()
        os.chdir(os.path.join(ROOT, "scripts"))
        try:
            return cli.CustomLightningCLI(args=["fit", "-c", "../configs/train_lfo_pairs_flanger_head.yml"], run=False,
                                          device=CPU, allow_missing_ckpt=True)
        finally:
            os.chdir(old)

    c = build()
    assert isinstance(c.model, lightning.LFOExtractionThroughEffect) and isinstance(c.model.model, models.Spectral2DCNN)
    assert isinstance(c.datamodule, data_modules.RandomAudioChunkDryWetDataModule)
    assert c.model.effect == "flanger" and c.model.audio_loss_dict == {"mrstft": 1.0} and c.model.learned_fx is None
    head = c.model.fx_head
    assert isinstance(head, fx.FxParamHead) and head.names == ["flanger.feedback", "flanger.depth"] and head.in_ch == 64
    assert head.fixed == {("flanger", "mix"): 1.0, ("flanger", "width"): 1.0, ("flanger", "min_delay_width"): 0.5}
    assert c.model.missing_fx_params(None, 64) == []                          # trains on (dry, wet, None, None)
    assert sum(p.numel() for p in c.model.parameters()) == 1340353 + 2 * 64 + 2
    sd = c.model.state_dict()
    assert "fx_head.weight" in sd and "fx_head.bias" in sd and not any(k.startswith("fx_head.tab") for k in sd)
    with torch.no_grad():
        head.weight.add_(0.25)
        head.bias.add_(0.5)
    sd = {k: v.clone() for k, v in c.model.state_dict().items()}
    again = build()
    assert not torch.equal(again.model.fx_head.weight, head.weight)
    again.model.load_state_dict(sd, strict=True)
    assert torch.equal(again.model.fx_head.weight, head.weight) and torch.equal(again.model.fx_head.bias, head.bias)

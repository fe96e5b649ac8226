"""CPU: the surface of the learned effect parameters -- ``fx.LearnedFxParams``' construction checks, the two new C-ABI entry
points, ``LFOExtractionThroughEffect(learned_fx=...)``'s parameters, precedence and errors, the shipped config and the state
dict.  No device work."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
OK = {"min": 0.0, "max": 0.9, "init": 0.3}


def lf(spec, **kw):
    from mod_extraction_amd import fx
    return fx.LearnedFxParams(spec, **kw)


def test_names_and_order():
    m = lf({"phaser": {"mix": OK, "depth": OK}, "flanger": {"mix": OK, "feedback": OK, "width": 0.5}, "tremolo": {"mix": OK}})
    assert m.names == ["phaser.depth", "phaser.mix", "flanger.feedback", "flanger.mix", "tremolo.mix"]
    assert m.fixed == {("flanger", "width"): 0.5} and m.raw.shape == (5,) and m.raw.dtype == torch.float32
    assert [k for k, _ in m.named_parameters()] == ["raw"] and list(m.state_dict()) == ["raw"]
    assert m.learned("flanger") == ("feedback", "mix") and m.covers("flanger", "width") and not m.covers("flanger", "depth")
    assert m.tab_i.dtype == torch.int32 and m.tab_i.tolist() == [[0] * 5, [3, 4, 2, 4, 4], [2, 2, 0, 0, 3]]
    assert lf({"phaser": {"centre_frequency_hz": {"min": 200.0, "max": 4000.0, "init": 1000.0}}}).tab_i[0].tolist() == [1]
    assert lf({"phaser": {"centre_frequency_hz": {"min": 200.0, "max": 4000.0, "init": 1000.0, "scale": "lin"}}}).tab_i[0].tolist() == [0]


@pytest.mark.parametrize("spec", [
    {"wah": {"mix": OK}},                                                           # an unknown kind
    {"dry": {"mix": OK}},                                                           # "dry" has no parameter
    {"tremolo": {"depth": OK}},                                                     # a name the kind does not have
    {"flanger": {"rate_hz": OK}},
    {"flanger": {"depth": {"min": 0.0, "max": 1.0, "init": 0.0}}},                  # min < init < max
    {"flanger": {"depth": {"min": 0.0, "max": 1.0, "init": 1.0}}},
    {"flanger": {"depth": {"min": 0.6, "max": 0.4, "init": 0.5}}},
    {"flanger": {"depth": {"min": 0.0, "max": 1.0}}},                               # no init
    {"flanger": {"feedback": {"min": 0.0, "max": 1.0, "init": 0.5}}},               # the flanger's feedback: max < 1
    {"chorus": {"feedback": {"min": 0.0, "max": 1.0, "init": 0.5}}},
    {"flanger": {"feedback": {"min": -0.1, "max": 0.9, "init": 0.5}}},              # and min >= 0
    {"flanger": {"width": {"min": 0.0, "max": 1.5, "init": 0.5}}},
    {"phaser": {"feedback": {"min": -1.0, "max": 0.9, "init": 0.0}}},               # the phaser's feedback: inside (-1, 1)
    {"phaser": {"feedback": {"min": -0.9, "max": 1.0, "init": 0.0}}},
    {"phaser": {"centre_frequency_hz": {"min": 0.0, "max": 4000.0, "init": 1000.0, "scale": "lin"}}},   # centre > 0
    {"phaser": {"centre_frequency_hz": {"min": 0.0, "max": 4000.0, "init": 1000.0}}},
    {"phaser": {"depth": {"min": 0.0, "max": 1.0, "init": 0.5, "scale": "log"}}},   # a log scale with min <= 0
    {"phaser": {"depth": {"min": 0.1, "max": 1.0, "init": 0.5, "scale": "cubic"}}},
    {"tremolo": {"mix": 1.5}},                                                      # a fixed number outside the range
    {"flanger": {"feedback": 1.0}},
    {"flanger": {"width": 0.5}},                                                    # nothing learned
    {},
])
def test_construction_errors(spec):
    with pytest.raises(ValueError):
        lf(spec)


def test_more_than_16_entries_and_raw_gain():
    full = {"flanger": {n: OK for n in ("feedback", "min_delay_width", "width", "depth", "mix")},
            "chorus": {n: OK for n in ("feedback", "min_delay_width", "width", "depth", "mix")},
            "tremolo": {"mix": OK},
            "phaser": {"depth": OK, "feedback": OK, "mix": OK, "centre_frequency_hz": {"min": 200.0, "max": 4000.0, "init": 1000.0}}}
    assert lf(full).raw.shape == (15,)                      # every (kind, name) pair there is
    # the step's kinds may repeat a family, a spec may not: 16 is reachable only through the API's limit itself
    from mod_extraction_amd import fx
    assert fx.FX_MAX_LEARNED == 16
    old = fx.FX_MAX_LEARNED
    try:
        fx.FX_MAX_LEARNED = 14
        with pytest.raises(ValueError):
            lf(full)
    finally:
        fx.FX_MAX_LEARNED = old
    for bad in (0.0, -1.0, float("inf")):
        with pytest.raises(ValueError):
            lf({"tremolo": {"mix": OK}}, raw_gain=bad)
    a, b = lf({"tremolo": {"mix": OK}}), lf({"tremolo": {"mix": OK}}, raw_gain=4.0)
    assert abs(float(a.raw) - 4.0 * float(b.raw)) < 1e-6 and abs(float(b.values()) - 0.3) < 1e-7


def test_abi_has_the_two_entry_points():
    from mod_extraction_amd import _hip, build
    from tests.test_abi import header_arg_counts
    lib = ctypes.CDLL(build.build(verbose=False))
    counts = header_arg_counts()
    for name, n in (("mx_fx_params_expand", 18), ("mx_fx_params_grad", 13)):
        assert hasattr(lib, name) and counts[name] == n == len(_hip.SIGNATURES[name]), name
    assert _hip.ABI_VERSION == 21 == lib.mx_abi_version()                    # (tests/test_abi.py pins the number of entry points)
    # arguments are checked before any launch: P = 17 is refused without a device
    lib2 = _hip.load()
    one = ctypes.c_void_p(8)
    rc = lib2.mx_fx_params_expand(one, one, one, 17, 1.0, one, None, None, 4, None, None, one, None, None, None, None, None, None)
    assert rc == -2
    assert lib2.mx_fx_params_grad(one, one, one, one, 17, 1.0, one, one, one, 4, 1.0, one, None) == -2
    assert lib2.mx_fx_params_expand(one, one, one, 2, 1.0, one, None, None, 4, one, None, None, None, None, None, None, None,
                                    None) == -1              # an lfo_scale output without its sample counts


def step_of(effect, **kw):
    from mod_extraction_amd import lightning
    return lightning.LFOExtractionThroughEffect(torch.nn.Linear(3, 2), effect=effect, **kw)


def test_default_adds_no_parameter():
    plain = step_of("flanger")
    assert plain.learned_fx is None and plain.step_metric_names == []
    assert [k for k, _ in plain.named_parameters()] == ["model.weight", "model.bias"]
    assert list(plain.state_dict()) == ["model.weight", "model.bias"]
    spec = {"flanger": {"feedback": OK, "mix": OK, "width": 1.0}}
    step = step_of("flanger", learned_fx=spec)
    assert [k for k, _ in step.named_parameters()] == ["model.weight", "model.bias", "learned_fx.raw"]
    assert step.step_metric_names == ["fx/flanger.feedback", "fx/flanger.mix"]
    from mod_extraction_amd import fx, trainer
    assert trainer.metric_names(step, "train") == ["train/mrstft", "train/loss", "fx/flanger.feedback", "fx/flanger.mix"]
    assert trainer.metric_names(step, "val") == ["val/mrstft", "val/loss"]
    assert trainer.metric_names(plain, "train") == ["train/mrstft", "train/loss"]
    module = fx.LearnedFxParams(spec, raw_gain=2.0)
    assert step_of("flanger", learned_fx=module).learned_fx is module        # a module is taken as it is
    with pytest.raises(ValueError):
        step_of("tremolo", learned_fx=spec)                                  # a kind the step does not have
    with pytest.raises(ValueError):
        step_of(("flanger", "phaser"), learned_fx={"chorus": {"mix": OK}})
    with pytest.raises(ValueError):
        step_of("flanger", learned_fx={"flanger": {"feedback": {"min": 0.0, "max": 1.0, "init": 0.5}}})


def test_missing_names_raise_a_value_error_that_names_them():
    spec = {"flanger": {"feedback": OK, "depth": OK, "mix": OK, "width": 1.0}}             # no min_delay_width
    step = step_of("flanger", learned_fx=spec)
    assert step.missing_fx_params(None, 4) == ["flanger.min_delay_width"]
    assert step.missing_fx_params({"min_delay_width": 0.5}, 4) == []
    dry = torch.zeros(4, 1, 64)
    with pytest.raises(ValueError, match="flanger.min_delay_width"):
        step.common_step((dry, dry, None, None), is_training=True)
    with pytest.raises(ValueError, match="flanger.min_delay_width"):
        step.clip_constants(None, 4, CPU)
    plain = step_of(("tremolo", "dry"))
    with pytest.raises(ValueError, match="tremolo.mix"):                                    # the old assert, as that rule
        plain.common_step((dry, dry, None, None), is_training=True)
    with pytest.raises(ValueError, match="tremolo.mix"):
        plain.clip_constants({}, 4, CPU)
    mixed = step_of(("flanger", "phaser", "dry"), learned_fx={"phaser": {"depth": OK}})
    assert mixed.missing_fx_params(None, 1) == ["flanger.feedback", "flanger.min_delay_width", "flanger.width", "flanger.depth",
                                                "flanger.mix"]                              # a batch without a phaser row
    assert "phaser.depth" not in mixed.missing_fx_params(None, 3) and "phaser.mix" in mixed.missing_fx_params(None, 3)


def test_check_fx_params_covers_what_the_batch_still_supplies():
    """The ranges are checked on the names still read from the batch, on the rows of the kind that reads them; the launch
    itself has no CPU fallback."""
    from mod_extraction_amd import _hip
    step = step_of(("flanger", "tremolo"), learned_fx={"flanger": {"feedback": OK}}, check_fx_params=True)
    fxp = {k: torch.full((4,), 0.5) for k in ("min_delay_width", "width", "depth", "mix")}
    with pytest.raises(_hip.HipLibraryError):
        step.clip_constants(fxp, 4, CPU)                                     # in range: reaches the launch
    bad = dict(fxp, depth=torch.tensor([0.5, 7.0, 1.5, 7.0]))                # row 2 is a flanger row, rows 1 and 3 are not
    with pytest.raises(AssertionError):
        step.clip_constants(bad, 4, CPU)
    with pytest.raises(_hip.HipLibraryError):
        step.clip_constants(dict(fxp, depth=torch.tensor([0.5, 7.0, 0.5, 7.0])), 4, CPU)   # the tremolo rows do not read depth


def test_shipped_config_and_state_dict():
    from mod_extraction_amd import cli, data_modules, fx, lightning, models
    old = os.getcwd()
    os.chdir(os.path.join(ROOT, "scripts"))
    try:
        c = cli.CustomLightningCLI(args=["fit", "-c", "../configs/train_lfo_pairs_flanger.yml"], run=False, device=CPU,
                                   allow_missing_ckpt=True)
    finally:
        os.chdir(old)
    assert isinstance(c.model, lightning.LFOExtractionThroughEffect) and isinstance(c.model.model, models.Spectral2DCNN)
    assert isinstance(c.datamodule, data_modules.RandomAudioChunkDryWetDataModule)
    assert c.model.effect == "flanger" and c.model.audio_loss_dict == {"mrstft": 1.0}
    lfx = c.model.learned_fx
    assert isinstance(lfx, fx.LearnedFxParams) and lfx.names == ["flanger.feedback", "flanger.depth", "flanger.mix"]
    assert lfx.fixed == {("flanger", "width"): 1.0, ("flanger", "min_delay_width"): 0.5}
    assert c.model.missing_fx_params(None, 64) == []                          # trains on (dry, wet, None, None)
    P = lfx.raw.numel()
    assert P == 3 and sum(p.numel() for p in c.model.parameters()) == 1340353 + P
    sd = c.model.state_dict()
    assert "learned_fx.raw" in sd and not any(k.startswith("learned_fx.tab") for k in sd)
    with torch.no_grad():
        lfx.raw.add_(0.25)
    sd = {k: v.clone() for k, v in c.model.state_dict().items()}
    os.chdir(os.path.join(ROOT, "scripts"))
    try:
        again = cli.CustomLightningCLI(args=["fit", "-c", "../configs/train_lfo_pairs_flanger.yml"], run=False, device=CPU,
                                       allow_missing_ckpt=True)
    finally:
        os.chdir(old)
    assert not torch.equal(again.model.learned_fx.raw, lfx.raw)
    again.model.load_state_dict(sd, strict=True)
    assert torch.equal(again.model.learned_fx.raw, lfx.raw)

"""CPU: lightning.LFOExtractionThroughEffect with a SEQUENCE of kinds as ``effect`` (a batch that mixes effects) -- the
constructor's checks, the row lists and per-row geometry of the batcher's interleave rule, the constants formed with the
batcher's arithmetic, and the shipped config.  No device work: nothing is rendered."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
ID = torch.nn.Identity()


def step_of(effect, **kw):
    from mod_extraction_amd import lightning
    return lightning.LFOExtractionThroughEffect(ID, effect=effect, **kw)


def test_constructor_checks():
    from mod_extraction_amd import fx
    step = step_of(("flanger", "chorus", "phaser"))
    assert step.effect == step.kinds == ("flanger", "chorus", "phaser")
    assert step_of(["tremolo", "dry"]).kinds == ("tremolo", "dry")                  # a list, as a YAML gives it
    with pytest.raises(ValueError):
        step_of(("flanger", "wah"))                                                 # an unknown kind
    with pytest.raises(ValueError):
        step_of(())                                                                 # an empty sequence
    too_long = 1000.0 * (fx.FLANGER_MAX_DELAY_SAMPLES + 1) / 44100                  # beyond the LDS limit
    with pytest.raises(ValueError):
        step_of(("flanger", "chorus"), chorus_max_min_delay_ms=too_long)
    with pytest.raises(ValueError):
        step_of(("flanger", "chorus"), max_lfo_delay_ms=too_long)
    with pytest.raises(ValueError):
        step_of(("chorus",), chorus_max_lfo_delay_ms=-1.0)
    step_of(("phaser", "tremolo"), max_min_delay_ms=-1.0, chorus_max_min_delay_ms=too_long)   # no such row: ignored
    with pytest.raises(NotImplementedError):
        step_of(("flanger", "phaser"), should_stretch=True)
    with pytest.raises(ValueError):
        step_of(("flanger", "phaser"), audio_loss_dict={"mrstft": 0.0, "esr": 0.0})
    with pytest.raises(NotImplementedError):
        step_of(("flanger", "phaser"), audio_loss_dict={"no_such_loss": 1.0})


def test_geometry_defaults():
    from mod_extraction_amd import data_modules, fx
    step = step_of(("flanger", "chorus", "phaser"))
    assert (step.max_min_delay_samples, step.max_lfo_delay_samples) == (44, 441)   # the flanger: 1 ms / 10 ms
    assert step.chorus_max_min_delay_ms == data_modules.CHORUS_FX["max_min_delay_ms"] == 30.0
    assert step.chorus_max_lfo_delay_ms == data_modules.CHORUS_FX["max_lfo_delay_ms"] == 10.0
    assert step.chorus_max_min_delay_samples == fx.delay_samples(30.0, 44100) == 1323
    assert step.chorus_max_lfo_delay_samples == 441
    other = step_of(("chorus",), chorus_max_min_delay_ms=20.0, chorus_max_lfo_delay_ms=5.0, sr=48000)
    assert (other.chorus_max_min_delay_samples, other.chorus_max_lfo_delay_samples) == (960, 240)


def test_string_effects_are_unchanged():
    """The attributes of the three single-effect steps as they were before ``effect`` took sequences."""
    want = {"flanger": (44, 441, 485), "tremolo": (0, 0, 0), "phaser": (0, 0, 0)}
    for effect, (mn, ml, m) in want.items():
        step = step_of(effect, audio_loss_dict={"mrstft": 1.0, "esr": 0.0}, loss_dict={"l1": 1.0})
        assert step.effect == effect and isinstance(step.effect, str) and step.kinds is None
        assert (step.max_min_delay_samples, step.max_lfo_delay_samples, step.max_delay_samples) == (mn, ml, m)
        assert (step.max_min_delay_ms, step.max_lfo_delay_ms) == (1.0, 10.0)
        assert step.loss_dict == {"mrstft": 1.0, "esr": 0.0, "lfo_l1": 1.0} and step.lfo_loss_dict == {"l1": 1.0}
        assert step.audio_loss_dict == {"mrstft": 1.0, "esr": 0.0}
        assert (step.sr, step.use_dry, step.model_smooth_n_frames, step.check_fx_params) == (44100, True, 0, False)
        assert not hasattr(step, "chorus_max_min_delay_samples")
    with pytest.raises(ValueError):
        step_of("wah")
    with pytest.raises(ValueError):
        step_of("chorus")                                                           # a kind of a sequence, not a family
    with pytest.raises(ValueError):
        step_of("flanger", max_min_delay_ms=-1.0)
    step_of("phaser", max_min_delay_ms=-1.0, max_lfo_delay_ms=1e6)


def test_row_assignment():
    from mod_extraction_amd import data_modules, lightning
    kinds = ("flanger", "chorus", "phaser")
    assert lightning.mixed_row_lists(kinds, 7) == {"delay": [0, 1, 3, 4, 6], "tremolo": [], "phaser": [2, 5], "dry": []}
    assert lightning.mixed_row_lists(kinds, 2) == {"delay": [0, 1], "tremolo": [], "phaser": [], "dry": []}   # no phaser row
    five = ("flanger", "chorus", "phaser", "tremolo", "dry")
    assert lightning.mixed_row_lists(five, 7) == {"delay": [0, 1, 5, 6], "tremolo": [3], "phaser": [2], "dry": [4]}
    step = step_of(kinds)
    m = step._mixed_rows(7, CPU)
    assert m["delay"].dtype == m["phaser"].dtype == m["tremolo"].dtype == torch.int32
    assert m["delay"].tolist() == [0, 1, 3, 4, 6] and m["phaser"].tolist() == [2, 5] and m["tremolo"].numel() == 0
    assert m["dry_idx"].dtype == torch.int64 and m["dry_idx"].numel() == 0
    assert step._mixed_rows(7, CPU) is m and step._mixed_rows(2, CPU) is not m       # cached per (B, device)
    assert step._mixed_rows(2, CPU)["phaser"].numel() == 0
    # the per-row geometry is the batcher's own, tensor for tensor
    m = step._mixed_rows(7, CPU)
    b = data_modules.SyntheticFxBatcher(7, 4410, 44100, kinds, CPU)
    assert b.kinds == [kinds[i % 3] for i in range(7)]
    assert torch.equal(m["max_delay"], b.max_delay) and m["max_delay"].dtype == torch.int32
    assert torch.equal(m["max_min_delay"], b.max_min_delay) and torch.equal(m["max_lfo_delay"], b.max_lfo_delay)
    assert m["max_delay_max"] == b.max_delay_max == 1323 + 441
    assert m["max_delay"].tolist() == [485, 1764, 485, 485, 1764, 485, 485]
    assert torch.equal(b.rows_fx, m["delay"]) and torch.equal(b.rows_ph, m["phaser"])
    assert step_of(("phaser", "dry"))._mixed_rows(4, CPU)["max_delay_max"] == 0


def test_constants_are_the_batchers():
    """lfo_scale / min_delay are fp32 tensor products with the per-row sample counts, one_minus_mix is 1 - mix in fp32
    (SyntheticFxBatcher.render); only what the kinds present need is read from fx_params."""
    torch.manual_seed(0)
    B = 7
    step = step_of(("flanger", "chorus", "phaser"))
    fxp = {k: torch.rand(B) for k in ("feedback", "min_delay_width", "width", "depth", "mix")}
    fxp["centre_frequency_hz"] = 100.0 + 1000.0 * torch.rand(B)
    c = step.clip_constants(fxp, B, CPU)
    m = step._mixed_rows(B, CPU)
    assert set(c) == {"lfo_scale", "min_delay", "feedback", "depth", "mix", "one_minus_mix", "centre_frequency_hz"}
    assert torch.equal(c["lfo_scale"], fxp["width"] * m["max_lfo_delay"])
    assert torch.equal(c["min_delay"], fxp["min_delay_width"] * m["max_min_delay"])
    assert torch.equal(c["one_minus_mix"], 1.0 - fxp["mix"]) and torch.equal(c["mix"], fxp["mix"])
    assert all(v.dtype == torch.float32 and v.shape == (B,) and v.is_contiguous() for v in c.values())
    assert set(step_of(("tremolo", "dry")).clip_constants({"mix": fxp["mix"]}, B, CPU)) == {"mix", "one_minus_mix"}
    assert step_of(("dry",)).clip_constants({}, B, CPU) == {}
    # check_fx_params: each family's ranges on its own rows -- a feedback of 1 is refused on a flanger row (0) only
    checked = step_of(("flanger", "tremolo"), check_fx_params=True)
    fb = fxp["feedback"].clone()
    fb[1] = 1.0
    checked.clip_constants(dict(fxp, feedback=fb), B, CPU)                           # row 1 is a tremolo row
    fb[0] = 1.0
    with pytest.raises(AssertionError):
        checked.clip_constants(dict(fxp, feedback=fb), B, CPU)


def test_constants_table_against_the_kernel_side_tables():
    """``lightning.CLIP_CONSTS`` (key, fx_params name, reading families, transform) against fx.FX_CONSTS / FX_PARAM_NAMES /
    FX_NAME_SLOT, and the keys of ``clip_constants`` against it for every combination of families present."""
    import itertools
    from mod_extraction_amd import fx, lightning
    table = lightning.CLIP_CONSTS
    keys = [row[0] for row in table]
    assert len(keys) == len(set(keys)) == len(fx.FX_CONSTS) and set(keys) == set(fx.FX_CONSTS)
    assert keys == ["mix", "one_minus_mix", "feedback", "depth", "lfo_scale", "min_delay", "centre_frequency_hz"]
    name_of = {row[0]: row[1] for row in table}
    readers = {row[0]: tuple(row[2]) for row in table}
    family = {"flanger": "delay", "chorus": "delay", "tremolo": "tremolo", "phaser": "phaser"}
    for kind, names in fx.FX_PARAM_NAMES.items():
        for name in names:
            assert name_of[fx.FX_NAME_SLOT[name]] == name and family[kind] in readers[fx.FX_NAME_SLOT[name]], (kind, name)
    assert name_of["one_minus_mix"] == "mix" and set(readers["one_minus_mix"]) == {"delay", "tremolo"} <= set(readers["mix"])
    assert all(set(r) <= {"delay", "tremolo", "phaser"} for r in readers.values())
    B = 5
    fxp = {"feedback": 0.3, "min_delay_width": 0.7, "width": 0.1, "depth": 0.9, "mix": 0.6, "centre_frequency_hz": 1300.1}
    five = ("flanger", "chorus", "phaser", "tremolo", "dry")
    effects = [c for n in range(1, 6) for c in itertools.combinations(five, n)] + ["flanger", "tremolo", "phaser"]
    seen = set()
    for effect in effects:
        step = step_of(effect)
        lists = step._mixed_rows(B, CPU)["lists"]
        want = [k for k in keys if any(lists[f] for f in readers[k])]
        assert list(step.clip_constants(fxp, B, CPU)) == want, effect
        seen.add(tuple(f for f in ("delay", "tremolo", "phaser") if lists[f]))
    assert len(seen) == 8                                                           # every combination of families, none included


def test_shipped_config_builds_its_object_graph():
    from mod_extraction_amd import cli, data_modules, lightning, models, optim
    old = os.getcwd()
    os.chdir(os.path.join(ROOT, "scripts"))
    try:
        c = cli.CustomLightningCLI(args=["fit", "-c", "../configs/train_lfo_interwoven_audio.yml"], run=False, device=CPU,
                                   allow_missing_ckpt=True)
    finally:
        os.chdir(old)
    assert isinstance(c.model, lightning.LFOExtractionThroughEffect) and isinstance(c.model.model, models.Spectral2DCNN)
    assert c.model.kinds == ("flanger", "chorus", "phaser") == tuple(c.datamodule.kinds)
    assert c.model.model.n_frames == 345 and c.model.model.in_ch == 2
    assert c.model.audio_loss_dict == {"mrstft": 1.0} and c.model.loss_dict == {"mrstft": 1.0}
    assert isinstance(c.datamodule, data_modules.InterwovenDataModule) and c.datamodule.batch_size == 256
    assert cli.resolve_class(c.optimizer_spec["class_path"]) is optim.FlatAdamW
    assert sum(p.numel() for p in c.model.parameters()) == 1340353
    assert c.trainer.max_epochs == 400


@pytest.mark.parametrize("effect", ["flanger", "tremolo", "phaser"])
def test_string_effect_constants_are_fx_derive(effect):
    """One rule for the constants: a string effect's are those of its ``fx.derive_*``, key for key and bit for bit, for
    tensor parameters (they meet the sample counts in fp32) and for python floats (in double, rounded once)."""
    from mod_extraction_amd import fx
    torch.manual_seed(1)
    B = 5
    step = step_of(effect)
    as_tensors = {k: torch.rand(B) for k in ("feedback", "min_delay_width", "width", "depth", "mix")}
    as_tensors["centre_frequency_hz"] = 100.0 + 1000.0 * torch.rand(B)
    as_floats = {"feedback": 0.3, "min_delay_width": 0.7, "width": 0.1, "depth": 0.9, "mix": 0.6, "centre_frequency_hz": 1300.1}
    for fxp in (as_tensors, as_floats):
        if effect == "flanger":
            want = fx.derive_clip_constants(B, CPU, 44, 441, fxp["feedback"], fxp["min_delay_width"], fxp["width"],
                                            fxp["depth"], fxp["mix"])
        elif effect == "tremolo":
            want = fx.derive_tremolo_constants(B, CPU, fxp["mix"])
        else:
            want = fx.derive_phaser_params(B, CPU, fxp["depth"], fxp["centre_frequency_hz"], fxp["feedback"], fxp["mix"])
        got = step.clip_constants(fxp, B, CPU)
        assert set(got) == set(want)
        for k in want:
            assert got[k].dtype == torch.float32 and got[k].is_contiguous() and torch.equal(got[k], want[k]), k
    # check_fx_params: the family owns every row, the ranges are checked on the parameters as they are
    checked = step_of(effect, check_fx_params=True)
    checked.clip_constants(as_tensors, B, CPU)
    checked.clip_constants(as_floats, B, CPU)
    for bad in (dict(as_tensors, mix=as_tensors["mix"] + 1.0), dict(as_floats, mix=1.5)):
        with pytest.raises(AssertionError):
            checked.clip_constants(bad, B, CPU)


def test_string_flanger_row_plan():
    """The row plan of a string effect: every row the one geometry, one family that owns all rows."""
    step = step_of("flanger")
    B = 6
    m = step._mixed_rows(B, CPU)
    assert torch.equal(m["max_delay"], torch.full((B,), 485, dtype=torch.int32)) and m["max_delay"].dtype == torch.int32
    assert m["max_delay_max"] == 485 == step.max_delay_samples
    assert m["delay"].tolist() == list(range(B)) and m["all_rows"] == "delay"
    assert step_of(("flanger", "chorus"))._mixed_rows(B, CPU)["all_rows"] == "delay"       # one family, two geometries
    assert step_of("tremolo")._mixed_rows(B, CPU)["all_rows"] == "tremolo"
    assert step_of("phaser")._mixed_rows(B, CPU)["all_rows"] == "phaser"
    assert step_of(("flanger", "phaser"))._mixed_rows(B, CPU)["all_rows"] is None
    assert step_of(("flanger", "phaser"))._mixed_rows(1, CPU)["all_rows"] == "delay"       # a batch without a phaser row
    assert step_of(("dry",))._mixed_rows(B, CPU)["all_rows"] is None

"""CPU: the arguments of lightning.LFOExtractionThroughEffect(effect=...) and the tremolo slots of the batcher's host-side
parameter draws (no device work: nothing is rendered here)."""
import numpy as np
import pytest
import torch


def test_tremolo_step_constructs_without_delay_arguments():
    from mod_extraction_amd import lightning
    step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), effect="tremolo")
    assert step.effect == "tremolo"
    # the delay arguments are ignored: values the flanger refuses are accepted
    lightning.LFOExtractionThroughEffect(torch.nn.Identity(), effect="tremolo", max_min_delay_ms=-1.0, max_lfo_delay_ms=1e6)
    with pytest.raises(ValueError):
        lightning.LFOExtractionThroughEffect(torch.nn.Identity(), max_min_delay_ms=-1.0)
    assert lightning.LFOExtractionThroughEffect(torch.nn.Identity()).effect == "flanger"


def test_unknown_effect_raises():
    from mod_extraction_amd import lightning
    with pytest.raises(ValueError):
        lightning.LFOExtractionThroughEffect(torch.nn.Identity(), effect="wah")


def test_should_stretch_still_raises():
    from mod_extraction_amd import lightning
    with pytest.raises(NotImplementedError):
        lightning.LFOExtractionThroughEffect(torch.nn.Identity(), effect="tremolo", should_stretch=True)


def draws(kinds, rng_order, seed=17, B=6, **kw):
    from mod_extraction_amd import data_modules
    torch.manual_seed(seed)
    np.random.seed(seed)
    batcher = data_modules.SyntheticFxBatcher(B, 4410, 44100, kinds, torch.device("cpu"), rng_order=rng_order, **kw)
    return batcher, batcher.sample_params()


FLANGER_PARAMS = ("feedback", "min_delay_width", "width", "depth", "mix")


def test_reference_order_tremolo_slots_next_to_flanger_dry():
    """rng_order="reference", ("flanger", "tremolo") against ("flanger", "dry") under one seed.

    A tremolo item draws rate, phase, shape and then its mix from the torch generator (datasets.py:367-372,492-495), so
    every torch draw AFTER the first tremolo item sits one value later in the stream than in the ("flanger", "dry") batch:
    the two batches share exactly (i) every rate (scipy's loguniform draws from the numpy stream, which the mix does not
    touch) and (ii) every draw up to and including the first tremolo item's shape -- the whole of flanger item 0.  The
    rest of the flanger draws is pinned against the reference's order written out by hand below, value for value."""
    from mod_extraction_amd import util
    B = 6
    bt, pt = draws(("flanger", "tremolo"), "reference", B=B)
    bd, pd = draws(("flanger", "dry"), "reference", B=B)
    assert torch.equal(pt["rate_hz"], pd["rate_hz"])
    assert pt["phase"][:2].tolist() == pd["phase"][:2].tolist() and pt["shape"][:2] == pd["shape"][:2]
    # the reference's order by hand: per item rate / phase / shape (/ mix), then the five (B,) flanger draws
    torch.manual_seed(17)
    np.random.seed(17)
    rate, phase, shape, mix = [], [], [], []
    for i in range(B):
        rate.append(util.sample_log_uniform(*bt.ms["rate_hz"]))
        phase.append(util.sample_uniform(*bt.ms["phase"]))
        shape.append(util.choice(list(bt.ms["shapes"])))
        mix.append(util.sample_uniform(0.0, 1.0) if i % 2 == 1 else None)
    five = {k: util.sample_uniform(*bt.fl[k], n=B) for k in FLANGER_PARAMS}
    assert pt["shape"] == shape
    assert torch.equal(pt["rate_hz"], torch.tensor(rate, dtype=torch.float64).float())
    assert torch.equal(pt["phase"], torch.tensor(phase, dtype=torch.float64).float())
    fl, tr = torch.arange(B) % 2 == 0, torch.arange(B) % 2 == 1
    for k in FLANGER_PARAMS:
        assert torch.equal(pt[k][fl], five[k][fl]), k
    assert torch.equal(pt["mix"][tr], torch.tensor([m for m in mix if m is not None], dtype=torch.float64).float())
    for k in ("feedback", "min_delay_width", "width", "depth"):
        assert float(pt[k][tr].abs().max()) == 0.0, k


def test_batch_order_flanger_draws_do_not_move():
    """rng_order="batch": the tremolo mix is the LAST draw, so every flanger draw equals the ("flanger", "dry") batch's."""
    _, pt = draws(("flanger", "tremolo"), "batch")
    _, pd = draws(("flanger", "dry"), "batch")
    fl = torch.arange(6) % 2 == 0
    for k in ("rate_hz", "phase") + FLANGER_PARAMS:
        assert torch.equal(pt[k][fl], pd[k][fl]), k
    assert torch.equal(pt["rate_hz"], pd["rate_hz"]) and pt["shape"] == pd["shape"]
    assert float(pt["mix"][~fl].min()) >= 0.0 and float(pt["mix"][~fl].max()) <= 1.0
    assert pt["mix"][~fl].unique().numel() == 3


def test_tremolo_mix_range_from_fx_config():
    bt, p = draws(("tremolo",), "batch", tremolo_fx={"mix": {"min": 0.25, "max": 0.5}})
    assert bt.tr["mix"] == (0.25, 0.5)
    assert float(p["mix"].min()) >= 0.25 and float(p["mix"].max()) <= 0.5
    bt, p = draws(("tremolo",), "reference", tremolo_fx={"mix": {"min": 0.25, "max": 0.5}})
    assert float(p["mix"].min()) >= 0.25 and float(p["mix"].max()) <= 0.5
    from mod_extraction_amd import data_modules
    assert data_modules.TremoloDataModule.kinds == ("tremolo",)
    assert data_modules.InterwovenDataModule.kinds == ("flanger", "chorus", "phaser")

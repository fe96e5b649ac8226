"""CPU: argument validation of lightning.LFOExtractionThroughEffect (the step that trains the extractor through the rendered
flanger with an audio loss).  No device is touched."""
import pytest
from torch import nn


def make(**kw):
    from mod_extraction_amd import lightning
    return lightning.LFOExtractionThroughEffect(nn.Linear(2, 2), **kw)


def test_defaults_and_metric_names():
    from mod_extraction_amd import lightning, trainer
    m = make(audio_loss_dict={"mrstft": 1.0, "l1": 0.0}, loss_dict={"l1": 0.5})
    assert isinstance(m, lightning.BaseLightingModule)
    assert m.max_delay_samples == 44 + 441
    assert trainer.metric_names(m, "train") == ["train/mrstft", "train/l1", "train/lfo_l1", "train/loss"]
    assert make().lfo_loss_dict == {}                                       # no supervised term by default


def test_unknown_audio_loss_with_weight_raises():
    with pytest.raises(NotImplementedError):
        make(audio_loss_dict={"mrstft": 1.0, "fdl1": 0.5})
    make(audio_loss_dict={"mrstft": 1.0, "fdl1": 0.0})                      # zero weight: only logged, accepted
    with pytest.raises(ValueError):
        make(audio_loss_dict={"mrstft": 0.0})                               # nothing to train on


def test_should_stretch_raises():
    with pytest.raises(NotImplementedError):
        make(should_stretch=True)


def test_geometry_is_checked():
    with pytest.raises(ValueError):
        make(max_min_delay_ms=0.0, max_lfo_delay_ms=0.0)                    # no delay line
    with pytest.raises(ValueError):
        make(max_min_delay_ms=30.0, max_lfo_delay_ms=800.0)                 # beyond the LDS budget of the kernels
    with pytest.raises(ValueError):
        make(max_min_delay_ms=-1.0)
    assert make(max_min_delay_ms=30.0, max_lfo_delay_ms=10.0).max_delay_samples == 1323 + 441

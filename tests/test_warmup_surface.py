"""CPU: the surface of the loss warm-up window of ``lightning.LFOExtractionThroughEffect(warmup_ms=...)`` -- the constructor's
validation, what ``None`` and 0 leave untouched, the ``ValueError`` of a window that leaves nothing, and the shipped config.
No device work."""
import math
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mk(**kw):
    from mod_extraction_amd import lightning
    return lightning.LFOExtractionThroughEffect(torch.nn.Identity(), **kw)


def test_constructor_validation(monkeypatch):
    from mod_extraction_amd import _hip, fx
    calls = []
    monkeypatch.setattr(_hip, "call", lambda name, *a: calls.append(name))
    for bad in (-1, -1e-9, math.inf, math.nan, "110", True, False, [110], (110,)):
        with pytest.raises(ValueError, match="warmup_ms"):
            mk(warmup_ms=bad)
    for ms, sr in ((110, 44100), (110.0, 44100), (50, 48000), (0.011, 44100), (0.012, 44100), (2000.0, 44100)):
        step = mk(warmup_ms=ms, sr=sr)
        assert step.warmup_ms == ms and step.warmup_samples == fx.delay_samples(ms, sr)
    assert mk(warmup_ms=110).warmup_samples == 4851 and mk(warmup_ms=0.011).warmup_samples == 0 and mk(warmup_ms=0.012).warmup_samples == 1
    assert calls == []


def test_none_and_zero_register_nothing():
    plain = mk()
    assert plain.warmup_ms is None and plain.warmup_samples == 0
    for kw in ({"warmup_ms": None}, {"warmup_ms": 0}, {"warmup_ms": 0.0}, {"warmup_ms": 110}, {"warmup_ms": 110, "match_fir": 5}):
        step = mk(**kw)
        assert list(step.state_dict()) == list(plain.state_dict()) and list(step.parameters()) == [] and list(step.buffers()) == []
        assert [n for n, _ in step.named_modules()] == [n for n, _ in plain.named_modules()]
        assert step.loss_dict == plain.loss_dict
        assert step.step_metric_names == (["fir/dc_gain", "fir/l1", "fir/flagged"] if "match_fir" in kw else [])
    assert mk(warmup_ms=0).warmup_samples == 0 and mk(warmup_ms=0)._warmup(1) == 0


def test_a_window_that_leaves_nothing_is_refused(monkeypatch):
    """P >= the samples the losses would see: a ValueError at the step, before any launch."""
    from mod_extraction_amd import _hip
    calls = []
    monkeypatch.setattr(_hip, "call", lambda name, *a: calls.append(name))
    step = mk(warmup_ms=110)                                                 # P = 4851
    assert step._warmup(4852) == 4851
    for n in (4851, 100):
        with pytest.raises(ValueError, match="warmup_ms = 110 is 4851 samples"):
            step._warmup(n)
    dry, wet = torch.zeros(2, 1, 4851), torch.zeros(2, 1, 4851)
    fxp = {k: 0.5 for k in ("feedback", "min_delay_width", "width", "depth", "mix")}
    with pytest.raises(ValueError, match="nothing is left"):
        step.audio_loss(torch.zeros(2, 10, requires_grad=True), dry, wet, fxp)
    with pytest.raises(ValueError, match="nothing is left"):
        with torch.no_grad():
            step.audio_loss(torch.zeros(2, 10), dry, wet, fxp)
    assert calls == []


def test_shipped_config():
    """train_lfo_pairs_flanger_warmup.yml is train_lfo_pairs_flanger_fir.yml plus ``warmup_ms: 110`` = ten delay lines of
    11 ms at the shipped geometry."""
    import yaml
    from mod_extraction_amd import cli, lightning
    load = lambda name: yaml.safe_load(open(os.path.join(ROOT, "configs", name)))
    new, base = load("train_lfo_pairs_flanger_warmup.yml"), load("train_lfo_pairs_flanger_fir.yml")
    assert new["model"]["init_args"].pop("warmup_ms") == 110
    assert new == base
    old = os.getcwd()
    os.chdir(os.path.join(ROOT, "scripts"))
    try:
        mk_cli = lambda name: cli.CustomLightningCLI(args=["fit", "-c", f"../configs/{name}"], run=False, device=torch.device("cpu"))
        c, b = mk_cli("train_lfo_pairs_flanger_warmup.yml"), mk_cli("train_lfo_pairs_flanger_fir.yml")
    finally:
        os.chdir(old)
    assert isinstance(c.model, lightning.LFOExtractionThroughEffect)
    assert c.model.warmup_ms == 110 and c.model.warmup_samples == 4851 and b.model.warmup_samples == 0
    assert c.model.warmup_samples == 10 * c.model.max_delay_samples + 1       # 485 samples a pass; 4851 from the rounding of 110 ms
    assert c.model.match_fir == 9 and c.model.step_metric_names == b.model.step_metric_names
    assert c.config["data"] == b.config["data"]
    assert {k: v for k, v in c.config["model"]["init_args"].items() if k != "warmup_ms"} == b.config["model"]["init_args"]
    assert c.model.warmup_samples < c.config["data"]["init_args"]["n_samples"]

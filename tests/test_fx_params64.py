"""CPU: the fp64 restatement of the learned effect parameters' map (tests/helpers/fx_params64.py) and
``fx.LearnedFxParams.values()`` against it.

* the helper's derivative against central finite differences in raw, lin and log scales, raw_gain 1 and 2.5: 1e-6 relative,
  the gate of the project's other fp64-versus-FD tests;
* ``values()`` is the helper's map of the stored raw: 1e-12 relative (fp64 against fp64);
* ``init`` is reproduced by ``values()`` at construction: to 1e-12 where logit(init) / raw_gain is an fp32 number (init the
  middle of a lin range, the geometric middle of a log range: raw = 0); for any other init the one rounding of raw to fp32
  moves the value by at most 2^-24 |raw| |d value / d raw|, and that bound (times 1.01 for the derivative taken at the rounded
  point) is the gate;
* the helper's reduction on a hand-made case."""
import numpy as np
import pytest
import torch

from tests.helpers import fx_params64 as h

SPEC = {"flanger": {"feedback": {"min": 0.0, "max": 0.95, "init": 0.3}, "depth": {"min": 0.1, "max": 1.0, "init": 0.5},
                    "width": {"min": 0.0, "max": 1.0, "init": 0.9}, "min_delay_width": 0.5, "mix": 1.0},
        "phaser": {"centre_frequency_hz": {"min": 200.0, "max": 4000.0, "init": 1000.0},
                   "feedback": {"min": -0.9, "max": 0.9, "init": -0.2},
                   "depth": {"min": 0.01, "max": 1.0, "init": 0.5, "scale": "log"}}}


def table(lf):
    f, i = lf.tab_f.numpy(), lf.tab_i.numpy()
    return f[0], f[1], i[0], i[1], i[2]


@pytest.mark.parametrize("gain", [1.0, 2.5])
def test_derivative_against_central_differences(gain):
    from mod_extraction_amd import fx
    lf = fx.LearnedFxParams(SPEC, raw_gain=gain)
    lo, hi, is_log, _, _ = table(lf)
    assert is_log.tolist() == [0, 0, 0, 1, 1, 0] and lf.names[3] == "phaser.depth"
    g = np.random.default_rng(3)
    for raw in (lf.raw.detach().double().numpy(), g.uniform(-3.0, 3.0, lo.size)):
        d = h.dvalue_draw(raw, lo, hi, is_log, gain)
        eps = 1e-5
        fd = (h.value(raw + eps, lo, hi, is_log, gain) - h.value(raw - eps, lo, hi, is_log, gain)) / (2 * eps)
        rel = np.abs(d - fd) / np.abs(fd)
        print(f"gain {gain}: max relative difference to central differences {rel.max():.3e}")
        assert float(rel.max()) <= 1e-6


@pytest.mark.parametrize("gain", [1.0, 2.5])
def test_values_is_the_helpers_map(gain):
    from mod_extraction_amd import fx
    lf = fx.LearnedFxParams(SPEC, raw_gain=gain)
    assert lf.raw.dtype == torch.float32 and lf.raw.shape == (6,) and isinstance(lf.raw, torch.nn.Parameter)
    lo, hi, is_log, slot, kind = table(lf)
    with torch.no_grad():
        lf.raw.copy_(torch.tensor([-6.0, -1.5, 0.0, 0.7, 3.0, 6.0]))
    got = lf.values()
    assert got.dtype == torch.float64 and got.shape == (6,)
    want = h.value(lf.raw.detach().double().numpy(), lo, hi, is_log, gain)
    rel = float(np.abs(got.detach().numpy() - want).max() / np.abs(want).max())
    assert rel <= 1e-12
    # autograd through values() is the helper's derivative
    got.sum().backward()
    d = h.dvalue_draw(lf.raw.detach().double().numpy(), lo, hi, is_log, gain)
    assert float(np.abs(lf.raw.grad.double().numpy() - d).max() / np.abs(d).max()) <= 1e-6   # raw.grad is fp32


@pytest.mark.parametrize("gain", [1.0, 2.5])
def test_init_is_reproduced(gain):
    from mod_extraction_amd import fx
    mid = {"flanger": {"feedback": {"min": 0.0, "max": 0.95, "init": 0.475}, "mix": {"min": 0.25, "max": 1.0, "init": 0.625}},
           "phaser": {"centre_frequency_hz": {"min": 250.0, "max": 4000.0, "init": 1000.0}}}
    lf = fx.LearnedFxParams(mid, raw_gain=gain)
    assert float(lf.raw.detach().abs().max()) < 1e-6                                          # logit(1/2) up to the ratio's rounding
    v = lf.values().detach().numpy()
    assert float(np.abs(v / np.asarray([0.475, 0.625, 1000.0]) - 1.0).max()) <= 1e-12
    lf = fx.LearnedFxParams(SPEC, raw_gain=gain)
    lo, hi, is_log, _, _ = table(lf)
    inits = np.asarray([0.3, 0.9, 0.5, 0.5, 1000.0, -0.2])
    assert lf.names == ["flanger.feedback", "flanger.width", "flanger.depth", "phaser.depth", "phaser.centre_frequency_hz",
                        "phaser.feedback"]
    raw = lf.raw.detach().double().numpy()
    bound = 1.01 * 2.0 ** -24 * np.abs(raw) * np.abs(h.dvalue_draw(raw, lo, hi, is_log, gain)) + 1e-12 * np.abs(inits)
    err = np.abs(lf.values().detach().numpy() - inits)
    print(f"gain {gain}: |values() - init| {err}, bound {bound}")
    assert bool((err <= bound).all())


def test_reduction_by_hand():
    # two entries: flanger.width (slot 0, scaled by the LFO sample count) and tremolo.mix (slot 4)
    lo, hi, is_log = np.asarray([0.0, 0.0]), np.asarray([1.0, 1.0]), np.asarray([0, 0])
    slot, kind = np.asarray([0, 4]), np.asarray([0, 3])
    row_kind = np.asarray([0, 3, 0, 4])
    grads = np.zeros((6, 4))
    grads[0] = [1.0, 100.0, -3.0, 100.0]
    grads[4] = [100.0, 2.0, 100.0, 100.0]
    d, mag = h.grad(grads, np.zeros(2), lo, hi, is_log, slot, kind, 1.0, row_kind, [10.0, 7.0, 20.0, 7.0], [1.0] * 4, scale=2.0)
    # sigmoid'(0) = 1/4: (1 * 10 - 3 * 20) / 4 * 2 and 2 / 4 * 2
    assert np.allclose(d, [-25.0, 1.0], rtol=0, atol=1e-15) and np.allclose(mag, [35.0, 1.0], rtol=0, atol=1e-15)
    e = h.expand(np.zeros(2), lo, hi, is_log, slot, kind, 1.0, row_kind, [10.0, 7.0, 20.0, 7.0], [1.0] * 4)
    assert e["lfo_scale"][1].tolist() == [True, False, True, False] and e["lfo_scale"][0].tolist() == [5.0, 0.0, 10.0, 0.0]
    assert e["mix"][1].tolist() == e["one_minus_mix"][1].tolist() == [False, True, False, False]
    assert e["one_minus_mix"][0][1] == 0.5 and not e["feedback"][1].any()

"""GPU: the phaser at depth 0 (constant cut-off: a linear time-invariant system) against its closed-form transfer function
(tests/helpers/fp64_refs.py:phaser_ir64 -- six first-order all-passes in a feedback loop, linear mix), which shares no
code with the kernels or with the C oracle.  Both kernels: the time-parallel scan (default) and the JUCE-order kernel
(exact_order=True).

The reference output is the fp64 impulse response convolved with the whole rendered source row (lead warm-up samples
included), cropped to the output window.  Gate per clip: max|y - y64| <= max(1e-5, 2 x max|orc_phaser - y64|) -- the
C oracle's own distance from the closed form measures what fp32 arithmetic (and the fp32 round trip of the cut-off
through log10 / pow, which dominates near the upper clamp with high feedback) costs on that clip.
"""
import itertools

import numpy as np
import pytest
import torch
from scipy.signal import fftconvolve

from tests.helpers import fp64_refs as R

pytestmark = pytest.mark.gpu

CENTRES = (5.0, 20.0, 70.0, 440.0, 5000.0, 18000.0, 25000.0)
FEEDBACKS = (0.0, 0.35, 0.7, -0.7, 0.9)
MIXES = (0.2, 1.0)
LEADS = (0, 3, 12345, 88200)
IR_LEN = 88200 + 88200


def _orc(x, centre, feedback, mix, sr):
    from oracle._cref import fptr, lib
    B, N = x.shape
    one = lambda v: np.full(B, v, np.float32)
    y = np.empty_like(x)
    lib().orc_phaser(fptr(np.ascontiguousarray(x)), fptr(one(1.0)), fptr(one(0.0)), fptr(one(centre)),
                     fptr(one(feedback)), fptr(one(mix)), B, N, float(sr), fptr(y), None)
    return y[0]


_IR = {}


def ir(centre, feedback, mix, sr):
    key = (centre, feedback, mix, sr)
    if key not in _IR:
        h, tail = R.phaser_ir64(centre, feedback, mix, sr, 1 << 20)
        assert tail < 1e-12, (key, tail)
        _IR[key] = h[:IR_LEN]
    return _IR[key]


def _launch(dev, src, params, lead, sr, N, exact_order):
    from mod_extraction_amd import fx
    d = lambda col: torch.tensor(col, dtype=torch.float32, device=dev)
    p = {"rate_hz": d([1.0] * len(params)), "depth": d([0.0] * len(params)),
         "centre_frequency_hz": d([q[0] for q in params]), "feedback": d([q[1] for q in params]),
         "mix": d([q[2] for q in params])}
    y = fx.phaser_forward(torch.from_numpy(src).to(dev), p, torch.tensor(lead, dtype=torch.int32, device=dev), sr, N,
                          exact_order=exact_order)
    return y.cpu().numpy()


@pytest.mark.parametrize("sr", [44100, 48000, 16000])
@pytest.mark.parametrize("N", [1000, 88200])
def test_phaser_depth0_matches_closed_form(dev, sr, N):
    params = list(itertools.product(CENTRES, FEEDBACKS, MIXES))
    B = len(params)
    lead = [LEADS[i % len(LEADS)] for i in range(B)]
    g = np.random.default_rng(sr + N)
    L = max(lead) + N
    amp = np.array([0.1 if abs(q[1]) >= 0.9 else 0.2 for q in params])[:, None]   # resonance of fb 0.9: peaks ~6x
    src = (g.uniform(-1, 1, (B, L)) * amp).astype(np.float32)
    y_scan = _launch(dev, src, params, lead, sr, N, False)
    y_juce = _launch(dev, src, params, lead, sr, N, True)
    worst = {"scan": 0.0, "juce": 0.0}
    for i, (c, fbk, mix) in enumerate(params):
        T = lead[i] + N
        x = src[i, :T]
        y64 = fftconvolve(x.astype(np.float64), ir(c, fbk, mix, sr)[:T])[lead[i]:T]
        assert np.abs(y64).max() < 0.95, (params[i], float(np.abs(y64).max()))     # no sample clips
        e_orc = float(np.abs(_orc(x[None], c, fbk, mix, sr)[lead[i]:] - y64).max())
        for name, y in (("scan", y_scan), ("juce", y_juce)):
            e = float(np.abs(y[i] - y64).max())
            assert e <= max(1e-5, 2.0 * e_orc), (name, params[i], lead[i], e, e_orc)
            worst[name] = max(worst[name], e / max(1e-5, 2.0 * e_orc))
    assert worst["scan"] <= 1.0
    assert worst["juce"] <= 1.0


@pytest.mark.parametrize("exact_order", [False, True])
def test_phaser_depth0_impulse_response(dev, exact_order):
    """A unit impulse at sample 0 (lead 0): the first 4097 output samples are h[0..4096] directly."""
    sr, N = 44100, 4097
    params = [(440.0, 0.7, 1.0), (70.0, -0.7, 0.2), (5000.0, 0.35, 1.0), (25000.0, 0.0, 1.0), (20.0, 0.9, 0.2)]
    src = np.zeros((len(params), N), dtype=np.float32)
    src[:, 0] = 0.5
    y = _launch(dev, src, params, [0] * len(params), sr, N, exact_order)
    for i, (c, fbk, mix) in enumerate(params):
        h = 0.5 * ir(c, fbk, mix, sr)[:N]
        e_orc = float(np.abs(_orc(src[i:i + 1], c, fbk, mix, sr) - h).max())
        e = float(np.abs(y[i] - h).max())
        assert e <= max(1e-5, 2.0 * e_orc), (params[i], e, e_orc)

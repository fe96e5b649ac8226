"""GPU: the kernels of csrc/fx_params.hip behind fx.fx_params_expand / fx_params_grad / fx.LearnedFxParams, against the numpy
fp64 restatement in tests/helpers/fx_params64.py.  One table throughout: every (kind, name) pair there is learned (15
entries: five each for the flanger and the chorus, one for the tremolo, four for the phaser; two log scales), raw drawn in
[-6, 6] with both ends present (saturation), raw_gain 1.5.

1. expand, B = 7 rows of kinds (flanger, chorus, phaser, tremolo, dry) cycling, the step's own sample counts.  The kernel
   evaluates the map in fp64 and rounds to fp32 once: <= 2^-24 relative, gated at 2^-23 (the fp64 exp / log of the device and
   of numpy differ by far less); lfo_scale / min_delay take one more fp32 multiply: 2^-22.  one_minus_mix is torch.equal to
   1.0 - mix of the kernel's own output.  Rows and slots without an entry keep a sentinel (the dry row everywhere,
   centre_frequency_hz on the flanger rows, lfo_scale on the phaser row, ...), and a NULL output is skipped.
2. grad, B = 1, 7 and 300 (more rows than the workgroup's 256 threads: loop and tail), per-row fp64 gradients over ten
   decades with mixed signs: |got - want| <= 6e-8 |want| + 1e-12 sum |terms| -- one fp32 cast of an fp64 sum, the gate of
   the project's fp64 gather kernels; rows of kinds without an entry hold NaN (they are never read); a second launch is
   torch.equal."""
import numpy as np
import pytest
import torch

from tests.helpers import fx_params64 as h

pytestmark = pytest.mark.gpu
FIVE = ("flanger", "chorus", "phaser", "tremolo", "dry")
GAIN = 1.5
UNIT = {"min": 0.0, "max": 1.0, "init": 0.5}
DELAY = {"feedback": {"min": 0.0, "max": 0.95, "init": 0.3}, "min_delay_width": UNIT, "width": UNIT, "depth": UNIT, "mix": UNIT}
SPEC = {"flanger": DELAY, "chorus": DELAY, "tremolo": {"mix": UNIT},
        "phaser": {"depth": {"min": 0.05, "max": 1.0, "init": 0.5, "scale": "log"}, "feedback": {"min": -0.9, "max": 0.9, "init": 0.1},
                   "centre_frequency_hz": {"min": 200.0, "max": 4000.0, "init": 1000.0}, "mix": UNIT}}


@pytest.fixture(scope="module")
def learned(dev):
    from mod_extraction_amd import fx
    lf = fx.LearnedFxParams(SPEC, raw_gain=GAIN).to(dev)
    assert len(lf.names) == 15
    raw = np.random.default_rng(16).uniform(-6.0, 6.0, 15)
    raw[0], raw[7], raw[12] = -6.0, 6.0, 6.0
    with torch.no_grad():
        lf.raw.copy_(torch.tensor(raw, dtype=torch.float32))
    return lf


def table(lf):
    f, i = lf.tab_f.cpu().numpy(), lf.tab_i.cpu().numpy()
    return lf.raw.detach().double().cpu().numpy(), f[0], f[1], i[0], i[1], i[2], GAIN


def rows_of(dev, B):
    kinds = [FIVE[i % 5] for i in range(B)]
    row_kind = torch.tensor([FIVE.index(k) for k in kinds], dtype=torch.int32, device=dev)
    ml = torch.tensor([441.0 if k in ("flanger", "chorus") else 0.0 for k in kinds], device=dev)
    mm = torch.tensor([1323.0 if k == "chorus" else 44.0 if k == "flanger" else 0.0 for k in kinds], device=dev)
    return kinds, row_kind, ml, mm


def test_expand(dev, learned):
    from mod_extraction_amd import fx
    B, S = 7, -7.0
    kinds, row_kind, ml, mm = rows_of(dev, B)
    consts = {k: torch.full((B,), S, device=dev) for k in fx.FX_CONSTS}
    values = learned.expand(consts, row_kind, ml, mm)
    want = h.expand(*table(learned), row_kind.cpu().numpy(), ml.cpu().numpy(), mm.cpu().numpy())
    for name in fx.FX_CONSTS:
        got = consts[name].double().cpu().numpy()
        ref, written = want[name]
        assert np.array_equal(got[~written], np.full(int((~written).sum()), S)), name          # the sentinel is kept
        assert written.any() and not written[4], name                                          # the dry row: never
        if name == "one_minus_mix":
            continue
        rel = float((np.abs(got - ref)[written] / np.abs(ref[written])).max())
        print(f"expand {name}: rows {np.nonzero(written)[0].tolist()}, max relative error {rel:.3e}")
        if name in ("lfo_scale", "min_delay"):
            assert rel <= 2.3841858e-07, name                                   # 2^-22
        else:
            assert rel <= 1.1920929e-07, name                                   # 2^-23
    assert want["centre_frequency_hz"][1].tolist() == [False, False, True, False, False, False, False]
    assert want["lfo_scale"][1].tolist() == [True, True, False, False, False, True, True]
    assert want["mix"][1].tolist() == [True, True, True, True, False, True, True]
    w = torch.tensor(want["mix"][1], device=dev)
    assert torch.equal(consts["one_minus_mix"][w], 1.0 - consts["mix"][w])
    vref = h.value(*table(learned)[:4], GAIN)
    rel = float((np.abs(values.double().cpu().numpy() - vref) / np.abs(vref)).max())
    print(f"expand values: max relative error {rel:.3e}")
    assert rel <= 1.1920929e-07                                                 # 2^-23
    # the saturated entries sit on (or within an ulp of) their range's end, which the effect still accepts
    assert float(values[7]) <= 1.0 and float(values[0]) >= 0.0 and float(consts["feedback"][0]) < 1.0
    # the two rows of one kind hold the same bits; a missing key (a NULL output) skips its slot
    assert all(torch.equal(v[0], v[5]) and torch.equal(v[1], v[6]) for v in consts.values())
    part = {k: torch.full((B,), S, device=dev) for k in ("mix", "depth")}
    again = learned.expand(part, row_kind, None, None)
    assert torch.equal(again, values) and torch.equal(part["mix"], consts["mix"]) and torch.equal(part["depth"], consts["depth"])


@pytest.mark.parametrize("B", [1, 7, 300])
def test_grad(dev, learned, B):
    _, row_kind, ml, mm = rows_of(dev, B)
    g = np.random.default_rng(100 + B)
    grads = g.choice([-1.0, 1.0], (6, B)) * 10.0 ** g.uniform(-5.0, 5.0, (6, B))
    want, mag = h.grad(grads, *table(learned), row_kind.cpu().numpy(), ml.cpu().numpy(), mm.cpu().numpy(), scale=0.75)
    # rows of kinds that have no entry for a slot are never read: poison them
    t = table(learned)
    covered = np.zeros((6, B), dtype=bool)
    for e in range(15):
        covered[t[4][e]] |= row_kind.cpu().numpy() == t[5][e]
    gd = torch.tensor(np.where(covered, grads, np.nan), device=dev)
    assert bool(torch.isnan(gd).any())
    got = learned.grad(gd, row_kind, ml, mm, scale=0.75)
    assert got.shape == (15,) and got.dtype == torch.float32 and torch.equal(got, learned.grad(gd, row_kind, ml, mm, scale=0.75))
    err = np.abs(got.double().cpu().numpy() - want)
    # err <= 6e-8 |want| + 1e-12 sum |terms|, written as one ratio so that the margin is on record
    worst = float((err / np.maximum(np.abs(want) + (1e-12 / 6e-8) * mag, 1e-300)).max())
    print(f"grad B {B}: worst error / (|want| + 1.67e-5 sum |terms|) {worst:.3e}; max |want| {np.abs(want).max():.3e}")
    assert worst <= 6e-8
    if B == 1:                                                                  # only the flanger has a row
        assert bool((got[5:] == 0).all()) and bool((got[:5] != 0).all())

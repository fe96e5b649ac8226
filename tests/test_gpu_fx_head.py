"""GPU: the kernels of csrc/fx_head.hip behind fx.fx_head_forward / fx_head_backward / fx.FxParamHead, against the numpy fp64
restatement in tests/helpers/fx_head64.py.  The 15-entry table, raw_gain 1.5 and the rows (kinds cycling over flanger, chorus,
phaser, tremolo, dry; the step's sample counts) of tests/test_gpu_fx_params.py.  Shapes (B, C, W): (7, 64, 345) the shipped
model's latent (an odd W: rows that are not 16-byte aligned), (7, 64, 1) one frame, (3, 5, 63) a C that is no multiple of the
wave count and a clip of C W = 315 floats (a misaligned clip base: scalar head and tail of the d_latent stores), (300, 64, 4)
more clips than a workgroup has threads.  The latent has mixed signs over five decades; weight and bias put raw at -6 and +6 in
one entry each (asserted) and inside about +-6 elsewhere.

Forward.  Every stage is one fp32 rounding of an fp64 evaluation of the fp32 stage before it, so each is compared with the
helper fed the KERNEL's previous stage:
  pooled     |got - want| <= 2^-23 |want| + 1e-12 sum_w |latent| / W    (one rounding; the fp64 sum's own error is ~1e-16 of
             the absolute terms)
  raw_rows   |got - want| <= 2^-23 |want| + 1e-12 (|bias| + sum_c |weight pooled|), against the fp64 dot of the kernel's pooled
  values and the constants: 2^-23 relative against the map of the kernel's raw_rows; lfo_scale / min_delay one more fp32
             multiply: 2^-22.  one_minus_mix is torch.equal to 1 - mix of the kernel's own output.
  Rows and slots without an entry keep a sentinel; a missing key (a NULL output) skips its slot.
  weight = 0: every constant vector and values[b] are torch.equal to what mx_fx_params_expand writes for raw = bias.
Backward, grads (6, B) over ten decades with mixed signs, NaN wherever no entry of the row's kind reads it:
  d_raw_rows, d_bias, d_weight and column 0 of d_latent: |got - want| <= 6e-8 |want| + 1e-12 sum |terms| -- one fp32 cast of an
  fp64 sum, the gate of tests/test_gpu_fx_params.py; d_latent is torch.equal along w to its column 0, exactly 0 on the dry
  rows and finite everywhere; a second launch is torch.equal."""
import numpy as np
import pytest
import torch

from tests.helpers import fx_head64 as hh
from tests.test_gpu_fx_params import GAIN, SPEC, rows_of

pytestmark = pytest.mark.gpu
SHAPES = [(7, 64, 345), (7, 64, 1), (3, 5, 63), (300, 64, 4)]
EPS23, EPS22 = 1.1920929e-07, 2.3841858e-07
SENTINEL = -7.0
_cases = {}


def case(dev, shape):
    """One forward launch per shape, shared (and left unchanged) by the tests that need it."""
    if shape in _cases:
        return _cases[shape]
    from mod_extraction_amd import fx
    B, C, W = shape
    head = fx.FxParamHead(SPEC, in_ch=C, raw_gain=GAIN).to(dev)
    assert len(head.names) == 15
    g = np.random.default_rng(1000 + B + C + W)
    latent = (g.choice([-1.0, 1.0], shape) * 10.0 ** g.uniform(-3.0, 2.0, shape)).astype(np.float32)
    pooled64 = latent.astype(np.float64).mean(-1)
    w0 = g.normal(0.0, 1.0, (15, C))
    weight = (w0 * (4.0 / np.abs(pooled64 @ w0.T).max())).astype(np.float32)
    bias = g.uniform(-1.5, 1.5, 15)
    dot = pooled64 @ weight.astype(np.float64).T
    bias[0], bias[7] = -6.0 - dot[0, 0], 6.0 - dot[0, 7]                     # raw[0, 0] = -6, raw[0, 7] = +6
    with torch.no_grad():
        head.weight.copy_(torch.tensor(weight))
        head.bias.copy_(torch.tensor(bias, dtype=torch.float32))
    kinds, row_kind, ml, mm = rows_of(dev, B)
    lat = torch.tensor(latent, device=dev)
    consts = {k: torch.full((B,), SENTINEL, device=dev) for k in fx.FX_CONSTS}
    pooled, raw_rows, values = head.forward_rows(lat, consts, row_kind, ml, mm)
    f, i = head.tab_f.cpu().numpy(), head.tab_i.cpu().numpy()
    c = {"head": head, "latent": lat, "latent_np": latent, "kinds": kinds, "row_kind": row_kind, "ml": ml, "mm": mm,
         "consts": consts, "pooled": pooled, "raw_rows": raw_rows, "values": values,
         "tab": (f[0], f[1], i[0], i[1], i[2]), "rk": row_kind.cpu().numpy(), "ml_np": ml.cpu().numpy(), "mm_np": mm.cpu().numpy()}
    _cases[shape] = c
    return c


def worst_ratio(got, want, terms, rel, floor=1e-12):
    """max of |got - want| / (|want| + (floor / rel) terms): <= rel is |got - want| <= rel |want| + floor terms."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    return float((err / np.maximum(np.abs(want) + (floor / rel) * terms, 1e-300)).max())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward(dev, shape):
    from mod_extraction_amd import fx
    B, C, W = shape
    c = case(dev, shape)
    head, consts = c["head"], c["consts"]
    lo, hi, is_log, slot, kind = c["tab"]
    assert c["pooled"].shape == (B, C) and c["raw_rows"].shape == c["values"].shape == (B, 15)
    assert all(t.dtype == torch.float32 for t in (c["pooled"], c["raw_rows"], c["values"]))
    # pooled
    want, terms = hh.pool(c["latent_np"])
    r = worst_ratio(c["pooled"].cpu().numpy(), want, terms / W, EPS23)
    print(f"{shape} pooled: worst error / (|want| + 8.4e-6 sum |terms| / W) {r:.3e}")
    assert r <= EPS23
    # raw_rows against the fp64 dot of the kernel's own pooled
    w64, b64 = head.weight.detach().double().cpu().numpy(), head.bias.detach().double().cpu().numpy()
    got_raw = c["raw_rows"].double().cpu().numpy()
    want, terms = hh.linear(c["pooled"].double().cpu().numpy(), w64, b64)
    r = worst_ratio(got_raw, want, terms, EPS23)
    print(f"{shape} raw_rows: worst error / (|want| + 8.4e-6 sum |terms|) {r:.3e}; raw in [{got_raw.min():.4f}, {got_raw.max():.4f}]")
    assert r <= EPS23
    assert abs(got_raw[0, 0] + 6.0) < 1e-3 and abs(got_raw[0, 7] - 6.0) < 1e-3 and got_raw.min() <= -5.999 and got_raw.max() >= 5.999
    # values and the constants against the map of the kernel's own raw_rows
    v64 = hh.values(got_raw, lo, hi, is_log, GAIN)
    rel = float((np.abs(c["values"].double().cpu().numpy() - v64) / np.abs(v64)).max())
    print(f"{shape} values: max relative error {rel:.3e}")
    assert rel <= EPS23
    want = hh.expand(v64, slot, kind, c["rk"], c["ml_np"], c["mm_np"])
    for name in fx.FX_CONSTS:
        got = consts[name].double().cpu().numpy()
        ref, written = want[name]
        assert np.array_equal(got[~written], np.full(int((~written).sum()), SENTINEL)), name      # the sentinel is kept
        dry_rows = c["rk"] == 4
        assert not written[dry_rows].any(), name
        if name == "one_minus_mix" or not written.any():
            continue
        rel = float((np.abs(got - ref)[written] / np.abs(ref[written])).max())
        print(f"{shape} {name}: {int(written.sum())} rows, max relative error {rel:.3e}")
        assert rel <= (EPS22 if name in ("lfo_scale", "min_delay") else EPS23), name
    w = torch.tensor(want["mix"][1], device=dev)
    assert bool(w.any()) and torch.equal(consts["one_minus_mix"][w], 1.0 - consts["mix"][w])
    assert want["centre_frequency_hz"][1].tolist() == [k == "phaser" for k in c["kinds"]]
    assert want["lfo_scale"][1].tolist() == [k in ("flanger", "chorus") for k in c["kinds"]]
    # rows of one kind get different values (the weight is at work)
    if B >= 7:
        assert not torch.equal(c["values"][0], c["values"][5])
    # a missing key (a NULL output) skips its slot; the rest has the same bits
    part = {k: torch.full((B,), SENTINEL, device=dev) for k in ("mix", "depth")}
    p2, r2, v2 = head.forward_rows(c["latent"], part, c["row_kind"], None, None)
    assert torch.equal(p2, c["pooled"]) and torch.equal(r2, c["raw_rows"]) and torch.equal(v2, c["values"])
    assert torch.equal(part["mix"], consts["mix"]) and torch.equal(part["depth"], consts["depth"])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_zero_weight_is_fx_params_expand(dev, shape):
    from mod_extraction_amd import fx
    B, C, W = shape
    c = case(dev, shape)
    head = c["head"]
    lf = fx.LearnedFxParams(SPEC, raw_gain=GAIN).to(dev)
    with torch.no_grad():
        lf.raw.copy_(head.bias)
    want = {k: torch.full((B,), SENTINEL, device=dev) for k in fx.FX_CONSTS}
    shared = lf.expand(want, c["row_kind"], c["ml"], c["mm"])
    got = {k: torch.full((B,), SENTINEL, device=dev) for k in fx.FX_CONSTS}
    zero = torch.zeros_like(head.weight)
    _, raw_rows, values = fx.fx_head_forward(c["latent"], zero, head.bias.detach(), head.tab_f, head.tab_i, GAIN, c["row_kind"],
                                             c["ml"], c["mm"], got)
    assert torch.equal(raw_rows, head.bias.detach().expand(B, 15))
    assert torch.equal(values, shared.expand(B, 15))
    for k in fx.FX_CONSTS:
        assert torch.equal(got[k], want[k]), k
    assert bool((got["feedback"] != SENTINEL).any())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward(dev, shape):
    from mod_extraction_amd import fx
    B, C, W = shape
    c = case(dev, shape)
    head = c["head"]
    lo, hi, is_log, slot, kind = c["tab"]
    g = np.random.default_rng(200 + B + W)
    grads = g.choice([-1.0, 1.0], (6, B)) * 10.0 ** g.uniform(-5.0, 5.0, (6, B))
    covered = np.zeros((6, B), dtype=bool)
    for e in range(15):
        covered[slot[e]] |= c["rk"] == kind[e]
    poisoned = np.where(covered, grads, np.nan)                              # rows no entry reads: never touched
    gd = torch.tensor(poisoned, device=dev)
    assert bool(torch.isnan(gd).any())
    args = (gd, c["raw_rows"], c["pooled"], head.weight.detach(), head.tab_f, head.tab_i, GAIN, c["row_kind"], c["ml"], c["mm"], W)
    d_rows, d_bias, d_weight, d_latent = fx.fx_head_backward(*args, scale=0.75, need_d_raw_rows=True)
    assert d_rows.shape == (B, 15) and d_bias.shape == (15,) and d_weight.shape == (15, C) and d_latent.shape == (B, C, W)
    assert all(t.dtype == torch.float32 for t in (d_rows, d_bias, d_weight, d_latent))
    want = hh.backward(poisoned, c["raw_rows"].double().cpu().numpy(), c["pooled"].double().cpu().numpy(),
                       head.weight.detach().double().cpu().numpy(), lo, hi, is_log, slot, kind, GAIN, c["rk"], c["ml_np"],
                       c["mm_np"], W, scale=0.75)
    for name, got in (("d_raw", d_rows), ("d_bias", d_bias), ("d_weight", d_weight), ("d_latent", d_latent[:, :, 0])):
        r = worst_ratio(got.cpu().numpy(), want[name], want["abs_" + name], 6e-8)
        print(f"{shape} {name}: worst error / (|want| + 1.67e-5 sum |terms|) {r:.3e}; max |want| {np.abs(want[name]).max():.3e}")
        assert r <= 6e-8, name
    assert bool(torch.isfinite(d_latent).all()) and torch.equal(d_latent, d_latent[:, :, :1].expand(B, C, W))
    dry = torch.tensor(c["rk"] == 4, device=dev)
    assert bool(dry.any()) or B < 5
    assert bool((d_latent[dry] == 0).all()) and bool((d_rows[dry] == 0).all())
    assert bool((d_latent[~dry] != 0).any())
    # the module's wrapper gives the same bits; so does a second launch; optional outputs may be left out
    again = fx.fx_head_backward(*args, scale=0.75, need_d_raw_rows=True)
    assert all(torch.equal(a, b) for a, b in zip(again, (d_rows, d_bias, d_weight, d_latent)))
    b2, w2, l2 = head.backward_rows(gd, c["raw_rows"], c["pooled"], c["row_kind"], c["ml"], c["mm"], W, scale=0.75,
                                    need_d_latent=False)
    assert l2 is None and torch.equal(b2, d_bias) and torch.equal(w2, d_weight)

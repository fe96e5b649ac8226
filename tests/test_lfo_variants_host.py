"""CPU: the batched LFO variants (csrc/lfo_variants.hip, modulations.make_quasi_periodic_batch / make_combined_mod_sigs and
the ``combined`` / ``quasiperiodic`` switches of data_modules.SyntheticFxBatcher) -- everything that needs no device.

* The SECTION-TABLE formulation the kernels implement (random draws in a fixed-width per-row table, consumed in corner
  order; sizes, offsets, truncation and tail stretch from a serial table; one output point at a time) is restated here in
  numpy on the oracle's ``find_corners`` / resampling / ``make_mod_signal`` and reproduces the REAL reference's outputs
  (tests/golden/eval_lfo_variants.npz) bit for bit, with the host stream replayed from the seeds of make_golden_misc.py.
* Table builders, unchanged parameter streams with the flags off, the flags of the three evaluation configs reaching the
  batcher, and the two ``ValueError``s.
``emulate_quasi`` / ``emulate_combined`` / ``replay_*`` are shared with tests/test_gpu_lfo_variants.py.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import modulations as omod, util as outil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
F32 = np.float32
S_GOLDEN = 16


def _golden_cases():
    spec = importlib.util.spec_from_file_location("make_golden_misc", os.path.join(ROOT, "tests", "golden", "make_golden_misc.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                       # definitions only: generation runs under __main__
    return mod.QUASI_CASES, mod.COMBINED_CASES


QUASI_CASES, COMBINED_CASES = _golden_cases()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "eval_lfo_variants.npz"))


# ---- the host stream of the reference, replayed into fixed-width tables -------------------------------------------
def replay_quasi_tables(seed, S, l_min, l_max, r_min, r_max, lr_split):
    """Per corner the reference draws ``torch.rand(1)`` for the split and then ``torch.rand(1)`` for the amount
    (util.sample_uniform twice, modulations.py:111-115); the table holds the first S corners' worth."""
    torch.manual_seed(seed)
    shrink, amount = np.zeros(S, np.int32), np.zeros(S, F32)
    for s in range(S):
        u_split = (torch.rand(1) * (1.0 - 0.0) + 0.0).item()
        shrink[s] = u_split < lr_split
        lo, hi = (l_min, l_max) if shrink[s] else (r_min, r_max)
        amount[s] = (torch.rand(1) * (hi - lo) + lo).item()
    return shrink, amount


def replay_combined_table(seed, S, shapes):
    """``torch.randint(0, len(shapes), (1,))`` per choice (util.choice): the base shape, then one per corner pair."""
    torch.manual_seed(seed)
    return [shapes[int(torch.randint(0, len(shapes), (1,)))] for _ in range(S + 1)]


# ---- the section-table formulation, one output point at a time ------------------------------------------------------
def corner_list(corner_map):
    return [int(i) for i in np.nonzero(corner_map == 1)[0]]


def select_corners(base):
    top, bot = omod.find_corners_np(base[None])
    return corner_list(top[0] if top.sum() > bot.sum() else bot[0])


def emulate_quasi(base, shrink, amount, S):
    base = np.asarray(base, F32)
    n = base.size
    corners = select_corners(base)
    m = len(corners)
    if m < 2 or m > S:
        return base.copy(), m
    src, n_in, n_out, off = [], [], [], []
    at, prev = 0, 0
    for s, c in enumerate(corners):
        size = c - prev + 1
        x = int(float(amount[s]) * size + 0.5)
        new = max(2, size - x) if shrink[s] else size + x
        src.append(prev); n_in.append(size); n_out.append(new); off.append(min(at, n))
        at += new - 1
        prev = c
    tail = n - prev
    total = at + tail
    src.append(prev); n_in.append(tail); n_out.append(tail + (n - total) if total < n else tail); off.append(min(at, n))
    off.append(n)
    out = np.empty(n, F32)
    resampled = {}
    for j in range(n):
        s = 0
        while s < m and off[s + 1] <= j:
            s += 1
        if s not in resampled:                        # the two taps of every point of the section, evaluated once
            resampled[s] = outil.linear_interpolate_last_dim_np(base[src[s]:src[s] + n_in[s]], n_out[s])
        out[j] = resampled[s][j - off[s]]
    return out, m


def emulate_combined(n, sr, freq, phase, shape_names, S):
    out = omod.make_mod_signal(n, sr, freq, phase, shape_names[0]).numpy().copy()
    _, bot = omod.find_corners_np(out[None])
    corners = corner_list(bot[0])
    m = len(corners)
    if m < 2:
        return out, m
    sections = {}
    for j in range(corners[0], corners[-1] + 1):
        seen = sum(1 for c in corners if c <= j)
        s = m - 2 if seen == m else seen - 1
        if s >= S:
            continue
        if s not in sections:
            length = corners[s + 1] - corners[s] + 1
            sections[s] = omod.make_mod_signal(length, length, 1.0, 0.0, shape_names[s + 1]).numpy()
        out[j] = sections[s][j - corners[s]]
    return out, m


def test_quasi_table_formulation_is_the_reference(golden):
    counts = []
    for i, (seed, shape, freq, phase, l0, l1, r0, r1, split) in enumerate(QUASI_CASES):
        base = omod.make_mod_signal(882, 441.0, freq, phase, shape).numpy()
        shrink, amount = replay_quasi_tables(seed, S_GOLDEN, l0, l1, r0, r1, split)
        out, m = emulate_quasi(base, shrink, amount, S_GOLDEN)
        assert np.array_equal(out, golden[f"quasi_{i}"]), i
        counts.append(m)
    assert counts[5] < 2 and counts[7] < 2 and max(counts) <= 6 and counts[0] == 5


def test_combined_table_formulation_is_the_reference(golden):
    counts = []
    for i, (seed, n, sr, freq, phase, shapes) in enumerate(COMBINED_CASES):
        names = replay_combined_table(seed, S_GOLDEN, list(shapes))
        out, m = emulate_combined(n, sr, freq, phase, names, S_GOLDEN)
        assert np.array_equal(out, golden[f"combined_{i}"]), i
        counts.append(m)
    assert counts[2] < 2 and counts[4] < 2 and max(counts) <= 6


def test_table_builders():
    from mod_extraction_amd import modulations as amod
    torch.manual_seed(3)
    shrink, amount = amod.draw_quasi_tables(7, 14, 0.1, 0.3333, 0.4, 0.5, 0.3)
    assert shrink.shape == amount.shape == (7, 14) and shrink.dtype == torch.int32 and amount.dtype == torch.float32
    assert set(shrink.unique().tolist()) == {0, 1}
    on = shrink.bool()
    assert bool(((amount[on] >= 0.1) & (amount[on] <= 0.3333)).all()) and bool(((amount[~on] >= 0.4) & (amount[~on] <= 0.5)).all())
    # two (B, S) draws, split first: the documented stream
    torch.manual_seed(3)
    u_split, u_amt = torch.rand(7, 14), torch.rand(7, 14)
    assert torch.equal(shrink.bool(), u_split.double() < 0.3)
    assert torch.equal(amount, torch.where(on, u_amt * (0.3333 - 0.1) + 0.1, u_amt * (0.5 - 0.4) + 0.4))
    names = ["tri", "rsaw", "cos"]
    torch.manual_seed(4)
    tab = amod.draw_combined_table(5, 9, names)
    torch.manual_seed(4)
    idx = torch.randint(0, 3, (5, 10))
    assert tab.shape == (5, 10) and tab.dtype == torch.int32
    assert tab.tolist() == [[amod.SHAPE_IDS[names[int(k)]] for k in row] for row in idx]
    torch.manual_seed(4)
    assert torch.equal(amod.draw_combined_table(5, 9, 3), idx.to(torch.int32))


def _batcher(mod_sig=None, kinds=("flanger",), **kw):
    from mod_extraction_amd import data_modules
    return data_modules.SyntheticFxBatcher(6, 88200, 44100, kinds, CPU, mod_sig=mod_sig, **kw)


def _seeded_params(b):
    torch.manual_seed(11)
    np.random.seed(11)
    return b.sample_params()


@pytest.mark.parametrize("kinds", [("flanger",), ("flanger", "chorus", "phaser"), ("tremolo", "dry")])
def test_streams_do_not_move_with_the_flags_off(kinds):
    """Flags off (absent, or written out as false with the default ranges): the draws of a batch are the parent's; flags
    on: every draw before the tables is still the same stream, the tables come last."""
    plain = _seeded_params(_batcher(None, kinds))
    off = _seeded_params(_batcher({"combined": False, "quasiperiodic": False, "l_min": 0.1, "l_max": 0.3, "r_min": 0.1,
                                   "r_max": 0.3, "lr_split": 0.5}, kinds))
    on_b = _batcher({"combined": True, "quasiperiodic": True}, kinds)
    on = _seeded_params(on_b)
    assert set(plain) == set(off) and set(on) - set(plain) == {"shape_table", "quasi_shrink", "quasi_amount"}
    for k, v in plain.items():
        for other in (off, on):
            assert torch.equal(v, other[k]) if isinstance(v, torch.Tensor) else v == other[k], k
    assert on["shape_table"].shape == (6, on_b.S + 1) and on["quasi_shrink"].shape == on["quasi_amount"].shape == (6, on_b.S)


def _config_batcher(name):
    from mod_extraction_amd import cli
    old = os.getcwd()
    os.chdir(os.path.join(ROOT, "scripts"))
    try:
        c = cli.CustomLightningCLI(args=["validate", "-c", os.path.join("..", "configs", name)], run=False, device=CPU,
                                   allow_missing_ckpt=True)
    finally:
        os.chdir(old)
    c.prepare_data_stream()
    return c, c.datamodule._batcher


def test_flags_of_the_evaluation_configs_reach_the_batcher():
    from mod_extraction_amd import data_modules, lightning
    c, b = _config_batcher("eval_lfo_quasi.yml")
    assert isinstance(c.datamodule, data_modules.FlangerCPUDataModule) and isinstance(c.model, lightning.LFOExtraction)
    assert b.quasiperiodic and not b.combined and b.quasi_args == (0.10, 0.3333, 0.10, 0.3333, 0.5)
    assert b.ms["rate_hz"] == (0.5, 2.0) and b.ms["exp"] == 1.0 and b.S == 2 * (int(2.0 * 88200 / 44100) + 2)
    assert b.fl["max_lfo_delay_ms"] == 4.0 and b.fl["feedback"] == (0.25, 0.25) and c.model.model_smooth_n_frames == 4
    c, b = _config_batcher("eval_lfo_combined.yml")
    assert b.combined and not b.quasiperiodic and b.ms["rate_hz"] == (1.0, 3.0) and b.ms["exp"] == 1.0
    assert b.S == 2 * (int(3.0 * 88200 / 44100) + 2) and b.quasi_args == (0.2, 0.2, 0.2, 0.2, 0.5)
    c, b = _config_batcher("eval_lfo_distorted.yml")
    assert not b.combined and not b.quasiperiodic and b.ms["exp"] == 2.0 and b.ms["rate_hz"] == (0.5, 3.0)
    assert float(b.sample_params()["exp"].min()) == 2.0
    for b in (_config_batcher("eval_lfo_quasi.yml")[1], _config_batcher("eval_lfo_combined.yml")[1]):
        assert list(b.ms["shapes"]) == ["cos", "tri", "rect_cos", "inv_rect_cos", "saw", "rsaw"]


def test_table_width_is_capped_at_the_kernel_limit():
    assert _batcher({"rate_hz": {"min": 0.5, "max": 40.0}}).S == 64


def test_reference_rng_order_refuses_the_variants():
    for flag in ("combined", "quasiperiodic"):
        with pytest.raises(ValueError):
            _batcher({flag: True}, rng_order="reference")
    _batcher({"combined": False, "quasiperiodic": False}, rng_order="reference")
    from mod_extraction_amd import data_modules
    dm = data_modules.FlangerCPUDataModule(4, fx_config={"mod_sig": {"quasiperiodic": True}}, rng_order="reference")
    with pytest.raises(ValueError):
        dm.setup(CPU)


def test_unknown_mod_sig_key_raises():
    with pytest.raises(ValueError, match="quasi_periodic"):
        _batcher({"quasi_periodic": True})

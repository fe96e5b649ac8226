"""GPU: the batched quasi-periodic / combined LFOs (csrc/lfo_variants.hip) and their use by the device batcher.

* ``mx_lfo_quasi_periodic`` against vectors of the REAL reference (tests/golden/eval_lfo_variants.npz, host stream replayed
  into the kernel's tables) and against the per-item device function ``modulations.make_quasi_periodic`` fed the same
  table values -- both bit for bit: the kernel only compares, does fp64 index arithmetic and evaluates the align_corners
  fma, all exactly rounded.
* ``mx_lfo_combined`` against the per-item ``make_combined_mod_sig`` bit for bit, and against the reference's vectors at
  1e-5 -- the gate tests/test_gpu_step.py applies to exactly these vectors (device ``cosf`` differs from the host's in the
  last ulp) -- with identical section boundaries.
* ``SyntheticFxBatcher`` with the settings of configs/eval_lfo_quasi.yml / eval_lfo_combined.yml: labels, the re-render
  property, phaser rows of an interwoven batch, the overlapped side stream, and ``validate`` end to end.
Every case is a handful of rows of 100 .. 1764 points.
"""
import os

import numpy as np
import pytest
import torch

from oracle import modulations as omod
from test_lfo_variants_host import (COMBINED_CASES, QUASI_CASES, S_GOLDEN, emulate_combined, replay_combined_table,
                                    replay_quasi_tables, select_corners)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ["cos", "tri", "rect_cos", "inv_rect_cos", "saw", "rsaw"]
QUASI_MS = {"rate_hz": {"min": 0.5, "max": 2.0}, "phase": {"min": 0.0, "max": 6.28318530718}, "shapes": SHAPES, "exp": 1.0,
            "quasiperiodic": True, "l_min": 0.10, "l_max": 0.3333, "r_min": 0.10, "r_max": 0.3333, "lr_split": 0.5}
COMBINED_MS = {"rate_hz": {"min": 1.0, "max": 3.0}, "phase": {"min": 0.0, "max": 6.28318530718}, "shapes": SHAPES,
               "exp": 1.0, "combined": True}
FLANGER = {"max_min_delay_ms": 1.0, "max_lfo_delay_ms": 4.0, "feedback": {"min": 0.25, "max": 0.25},
           "min_delay_width": {"min": 1.0, "max": 1.0}, "width": {"min": 1.0, "max": 1.0},
           "depth": {"min": 1.0, "max": 1.0}, "mix": {"min": 1.0, "max": 1.0}}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "eval_lfo_variants.npz"))


@pytest.fixture(scope="module")
def quasi_golden_inputs():
    """Bases of the 8 reference cases from the oracle (CPU) and the tables replayed from their seeds."""
    bases, shrink, amount, counts = [], [], [], []
    for seed, shape, freq, phase, l0, l1, r0, r1, split in QUASI_CASES:
        base = omod.make_mod_signal(882, 441.0, freq, phase, shape).numpy()
        sh, am = replay_quasi_tables(seed, S_GOLDEN, l0, l1, r0, r1, split)
        bases.append(base); shrink.append(sh); amount.append(am); counts.append(len(select_corners(base)))
    return np.stack(bases), np.stack(shrink), np.stack(amount), counts


# ---- mx_lfo_quasi_periodic ------------------------------------------------------------------------------------------
def test_quasi_batch_is_the_reference_bit_for_bit(dev, golden, quasi_golden_inputs):
    from mod_extraction_amd import modulations as amod
    bases, shrink, amount, counts = quasi_golden_inputs
    base_d = torch.from_numpy(bases).to(dev)
    out, nc = amod.make_quasi_periodic_batch(base_d, torch.from_numpy(shrink).to(dev), torch.from_numpy(amount).to(dev))
    out, nc = out.cpu().numpy(), nc.cpu().tolist()
    assert nc == counts and counts[0] == 5 and counts[5] < 2 and counts[7] < 2
    for i in range(len(QUASI_CASES)):
        assert np.array_equal(out[i], golden[f"quasi_{i}"]), i
    for i in (5, 7):                                           # fewer than 2 corners: unchanged
        assert np.array_equal(out[i], bases[i])
    # the same launch run again: identical bits
    again, _ = amod.make_quasi_periodic_batch(base_d, torch.from_numpy(shrink).to(dev), torch.from_numpy(amount).to(dev))
    assert np.array_equal(again.cpu().numpy(), out)


@pytest.mark.parametrize("S", [2, 1])
def test_quasi_rows_with_more_corners_than_table_entries_are_copied(dev, quasi_golden_inputs, S):
    from mod_extraction_amd import modulations as amod
    bases, shrink, amount, counts = quasi_golden_inputs
    out, nc = amod.make_quasi_periodic_batch(torch.from_numpy(bases).to(dev), torch.from_numpy(shrink[:, :S].copy()).to(dev),
                                             torch.from_numpy(amount[:, :S].copy()).to(dev))
    assert nc.cpu().tolist() == counts                         # the real count, so a caller can see it
    out = out.cpu().numpy()
    assert np.array_equal(out[0], bases[0])                    # case 0 has 5 corners
    for i, c in enumerate(counts):
        if c < 2 or c > S:
            assert np.array_equal(out[i], bases[i]), i
        else:                                                  # c == 2 == S: stretched
            assert not np.array_equal(out[i], bases[i]), i


def _per_item_quasi(amod, base_row, shrink_row, amount_row, monkeypatch):
    """``modulations.make_quasi_periodic`` with ``util.sample_uniform`` handing out the table values in section order."""
    from mod_extraction_amd import util as autil
    queue = []
    for s in range(len(shrink_row)):
        queue += [0.0 if int(shrink_row[s]) else 1.0, float(amount_row[s])]
    it = iter(queue)
    monkeypatch.setattr(autil, "sample_uniform", lambda low, high, n=1: next(it))
    return amod.make_quasi_periodic(base_row, 0.0, 0.0, 0.0, 0.0, 0.5)


QUASI_ROWS = [  # (n, sr, freq, phase, shape, table): table = (shrink, amount) for every section, or a seed
    (882, 441.0, 2.3, 0.4, "cos", (1, 0.99)),                 # the max(2, ...) floor: every section shrinks to 2 points
    (882, 441.0, 2.3, 0.4, "tri", (0, 0.5)),                  # all grow: truncated, later sections wholly beyond n
    (882, 441.0, 1.9, 1.0, "rect_cos", (1, 0.4)),             # all shrink: the tail is stretched
    (882, 441.0, 2.9, 5.0, "saw", 101),
    (882, 441.0, 0.3, 0.0, "cos", 102),                       # fewer than 2 corners
    (882, 441.0, 1.9, 2.2, "inv_rect_cos", 103),
    (100, 50.0, 2.3, 0.4, "cos", 104), (100, 50.0, 1.7, 3.0, "rsaw", (0, 0.5)),          # lengths that are no multiple of 64
    (345, 172.5, 2.9, 6.0, "tri", 105), (345, 172.5, 2.1, 1.0, "cos", (1, 0.4)),
]


def test_quasi_batch_equals_the_per_item_device_function(dev, monkeypatch):
    from mod_extraction_amd import modulations as amod
    S = 16
    stretched = 0
    for n in (882, 100, 345):
        rows = [r for r in QUASI_ROWS if r[0] == n]
        sr = rows[0][1]
        f = torch.tensor([r[2] for r in rows], device=dev)
        p = torch.tensor([r[3] for r in rows], device=dev)
        sh = torch.tensor([amod.SHAPE_IDS[r[4]] for r in rows], dtype=torch.int32, device=dev)
        base = amod.make_mod_signals(n, sr, f, p, sh)
        shrink, amount = torch.zeros(len(rows), S, dtype=torch.int32), torch.zeros(len(rows), S)
        for i, r in enumerate(rows):
            if isinstance(r[5], tuple):
                shrink[i], amount[i] = r[5]
            else:
                torch.manual_seed(r[5])
                shrink[i], amount[i] = (t[0] for t in amod.draw_quasi_tables(1, S, 0.05, 0.45, 0.05, 0.45, 0.5))
        out, nc = amod.make_quasi_periodic_batch(base, shrink.to(dev), amount.to(dev))
        assert out.shape == base.shape and int(nc.max()) <= S
        for i in range(len(rows)):
            want = _per_item_quasi(amod, base[i].clone(), shrink[i], amount[i], monkeypatch)
            assert want.shape == (n,) and torch.equal(out[i], want), (n, i)
            stretched += int(not torch.equal(out[i], base[i]))
    assert stretched == len(QUASI_ROWS) - 1                    # every row but the one with fewer than 2 corners


# ---- mx_lfo_combined ------------------------------------------------------------------------------------------------
def _per_item_combined(amod, n, sr, freq, phase, names, dev, monkeypatch):
    from mod_extraction_amd import util as autil
    it = iter(names)
    monkeypatch.setattr(autil, "choice", lambda items: next(it))
    return amod.make_combined_mod_sig(n, sr, freq, phase, SHAPES, device=dev)


def test_combined_batch_equals_the_per_item_device_function(dev, monkeypatch):
    from mod_extraction_amd import modulations as amod
    S = 16
    for n, sr, rows in ((882, 441.0, [(2.3, 0.4), (2.9, 5.0), (1.1, 2.0), (0.4, 1.0), (3.0, 6.1)]),
                        (345, 172.5, [(2.9, 6.0), (1.3, 0.2)]), (100, 50.0, [(2.3, 0.4)])):
        torch.manual_seed(n)
        tab = amod.draw_combined_table(len(rows), S, SHAPES)
        tab[0, 0] = amod.SHAPE_IDS["rect_cos"]                # the half-rate shapes as base and as section
        tab[0, 1:4] = torch.tensor([amod.SHAPE_IDS[s] for s in ("inv_rect_cos", "rect_cos", "saw")], dtype=torch.int32)
        f = torch.tensor([r[0] for r in rows], device=dev)
        p = torch.tensor([r[1] for r in rows], device=dev)
        out, nc = amod.make_combined_mod_sigs(n, sr, f, p, tab.to(dev))
        base = amod.make_mod_signals(n, sr, f, p, tab[:, 0].contiguous().to(dev))
        by_id = {v: k for k, v in amod.SHAPE_IDS.items()}
        for i, (freq, phase) in enumerate(rows):
            names = [by_id[int(k)] for k in tab[i]]
            want = _per_item_combined(amod, n, sr, freq, phase, names, dev, monkeypatch)
            assert torch.equal(out[i], want), (n, i)
            _, bot = amod.find_corners(base[i:i + 1])
            assert int(nc[i]) == int((bot == 1).sum())
            if int(nc[i]) < 2:
                assert torch.equal(out[i], base[i])
            else:
                assert not torch.equal(out[i], base[i])


def test_combined_pairs_beyond_the_table_keep_the_base(dev):
    from mod_extraction_amd import modulations as amod
    n, sr = 882, 441.0
    f, p = torch.tensor([2.9, 2.3], device=dev), torch.tensor([1.0, 0.4], device=dev)
    torch.manual_seed(5)
    tab = amod.draw_combined_table(2, 16, ["tri", "saw", "rsaw"])
    tab[:, 0] = amod.SHAPE_IDS["cos"]
    full, nc = amod.make_combined_mod_sigs(n, sr, f, p, tab.to(dev))
    base = amod.make_mod_signals(n, sr, f, p, tab[:, 0].contiguous().to(dev))
    _, bot = amod.find_corners(base)
    for S in (1, 2):
        cut, nc_s = amod.make_combined_mod_sigs(n, sr, f, p, tab[:, :S + 1].contiguous().to(dev))
        assert torch.equal(nc_s, nc) and int(nc.min()) >= 4
        for i in range(2):
            c = torch.nonzero(bot[i] == 1).view(-1).tolist()
            assert torch.equal(cut[i, :c[S]], full[i, :c[S]])          # sections 0 .. S-1, the shared corners included
            assert torch.equal(cut[i, c[S]:], base[i, c[S]:])          # corner S starts a pair the table does not hold
            assert not torch.equal(cut[i], full[i])


def test_combined_batch_against_the_reference_vectors(dev, golden):
    from mod_extraction_amd import modulations as amod
    worst = 0.0
    for i, (seed, n, sr, freq, phase, shapes) in enumerate(COMBINED_CASES):
        names = replay_combined_table(seed, S_GOLDEN, list(shapes))
        _, m = emulate_combined(n, sr, freq, phase, names, S_GOLDEN)     # the oracle's bottom-corner count
        tab = torch.tensor([[amod.SHAPE_IDS[s] for s in names]], dtype=torch.int32, device=dev)
        f, p = torch.tensor([freq], device=dev), torch.tensor([phase], device=dev)
        out, nc = amod.make_combined_mod_sigs(n, sr, f, p, tab)
        assert int(nc[0]) == m, i
        err = float(np.abs(out[0].cpu().numpy() - golden[f"combined_{i}"]).max())
        worst = max(worst, err)
        assert err < 1e-5, (i, err)
        if i in (2, 4):                                        # fewer than 2 bottom corners: the base
            assert m < 2 and torch.equal(out, amod.make_mod_signals(n, sr, f, p, tab[:, 0].contiguous()))
    print(f"[measured] batched combined LFOs vs reference vectors: max abs err {worst:.2e} (gate 1e-5)")


# ---- the batcher ----------------------------------------------------------------------------------------------------
def _flanger_batcher(dev, mod_sig, seed=7, B=8, overlap=False):
    from mod_extraction_amd import data_modules
    dm = data_modules.FlangerCPUDataModule(B, n_samples=88200, sr=44100, fx_config={"mod_sig": mod_sig, "flanger": FLANGER},
                                           overlap=overlap)
    torch.manual_seed(seed)
    np.random.seed(seed)
    dm.setup(dev, seed=seed)
    return dm._batcher


def _expected_label(b, p, fxp, dev):
    from mod_extraction_amd import modulations as amod
    shape_id = torch.tensor([amod.SHAPE_IDS[s] for s in fxp["shape"]], dtype=torch.int32, device=dev)
    plain = amod.make_mod_signals(b.n_lfo, b.lfo_sr, fxp["rate_hz"], fxp["phase"], shape_id, fxp["exp"])
    want, nc = plain, None
    if b.combined:
        want, nc = amod.make_combined_mod_sigs(b.n_lfo, b.lfo_sr, fxp["rate_hz"], fxp["phase"], p["shape_table"].to(dev))
    if b.quasiperiodic:
        want, nc = amod.make_quasi_periodic_batch(want, p["quasi_shrink"].to(dev), p["quasi_amount"].to(dev))
    return plain, want, nc


@pytest.mark.parametrize("which", ["quasi", "combined", "both"])
def test_batcher_renders_the_variants(dev, which):
    from mod_extraction_amd import fx
    ms = {"quasi": QUASI_MS, "combined": COMBINED_MS, "both": dict(QUASI_MS, combined=True)}[which]
    b = _flanger_batcher(dev, ms)
    assert b.S == 2 * (int(b.ms["rate_hz"][1] * 2) + 2)
    p = b.sample_params()
    dry, wet, mod, fxp = b.render(p)
    assert mod.shape == (8, 882) and dry.shape == wet.shape == (8, 1, 88200)
    assert set(fxp) == {"feedback", "min_delay_width", "width", "depth", "mix", "rate_hz", "phase", "shape", "exp",
                        "centre_frequency_hz", "lead"}                      # the tables are not part of fx_params
    plain, want, nc = _expected_label(b, p, fxp, dev)
    assert torch.equal(mod, want) and torch.equal(b.last_n_corners, nc)
    assert bool((b.last_n_corners <= b.S).all())
    changed = [not torch.equal(mod[i], plain[i]) for i in range(8)]
    many = (b.last_n_corners >= 2).cpu().tolist()
    assert sum(many) >= 2 and all(c for c, m in zip(changed, many) if m)
    assert float(mod.min()) >= 0.0 and float(mod.max()) <= 1.0 and bool(torch.isfinite(mod).all())
    # the re-render property: wet is the flanger of dry driven by the returned label
    consts = {"lfo_scale": (fxp["width"] * b.max_lfo_delay).contiguous(),
              "min_delay": (fxp["min_delay_width"] * b.max_min_delay).contiguous(),
              "feedback": fxp["feedback"], "depth": fxp["depth"], "mix": fxp["mix"],
              "one_minus_mix": (1.0 - fxp["mix"]).contiguous()}
    again = fx.flanger_forward(dry[:, 0, :], mod, consts, b.max_delay, b.max_delay_max)
    assert torch.equal(again, wet[:, 0, :])


def test_interwoven_phaser_rows_are_untouched_by_the_quasi_flag(dev):
    from mod_extraction_amd import data_modules
    got = {}
    for flag in (False, True):
        ms = dict(QUASI_MS, quasiperiodic=flag, rate_hz={"min": 0.5, "max": 3.0})
        dm = data_modules.InterwovenDataModule(6, shared_args={"n_samples": 88200, "sr": 44100},
                                               train_dataset_args=[{"fx_config": {"mod_sig": ms}}], overlap=False)
        torch.manual_seed(9)
        np.random.seed(9)
        dm.setup(dev, seed=9)
        assert dm._batcher.quasiperiodic is flag
        dry, wet, mod, fxp = dm.train_batch()
        got[flag] = (dry.clone(), wet.clone(), mod.clone(), fxp, dm._batcher.last_n_corners)
    ph, other = [2, 5], [0, 1, 3, 4]
    assert torch.equal(got[True][0], got[False][0])                        # the draws are appended: same stream before them
    assert torch.equal(got[True][2][ph], got[False][2][ph]) and torch.equal(got[True][1][ph], got[False][1][ph])
    for k in ("rate_hz", "phase", "depth", "feedback", "mix", "lead"):
        assert torch.equal(got[True][3][k], got[False][3][k]), k
    assert got[False][4] is None
    for i in other:
        if int(got[True][4][i]) >= 2:
            assert not torch.equal(got[True][2][i], got[False][2][i]) and not torch.equal(got[True][1][i], got[False][1][i])
    assert sum(int(got[True][4][i]) >= 2 for i in other) >= 2


def test_overlapped_batches_equal_the_serial_ones(dev):
    got = {}
    for overlap in (False, True):
        b = _flanger_batcher(dev, dict(QUASI_MS, combined=True), seed=13, B=4, overlap=overlap)
        assert b.overlap is overlap
        torch.manual_seed(13)
        np.random.seed(13)
        out = []
        for _ in range(2):
            dry, wet, mod, _ = b.next_batch()
            out.append((dry.clone(), wet.clone(), mod.clone(), b.last_n_corners.clone()))
        torch.cuda.synchronize()
        got[overlap] = out
    for a, c in zip(got[False], got[True]):
        for x, y in zip(a, c):
            assert torch.equal(x, y)
    assert not torch.equal(got[False][0][2], got[False][1][2])


def test_validate_runs_on_the_quasi_config(dev):
    """scripts/validate.py's path on configs/eval_lfo_quasi.yml (freshly initialised weights, one validation batch)."""
    import math
    from mod_extraction_amd import cli
    cwd = os.getcwd()
    os.chdir(os.path.join(ROOT, "scripts"))
    try:
        c = cli.CustomLightningCLI(args=["validate", "-c", "../configs/eval_lfo_quasi.yml"], run=False, device=dev,
                                   allow_missing_ckpt=True, trainer_defaults={"log_fn": None, "limit_val_batches": 1})
    finally:
        os.chdir(cwd)
    c.prepare_data_stream()
    assert c.datamodule._batcher.quasiperiodic and c.datamodule._batcher.S == 12
    c.model.eval()
    metrics = c.trainer.validate(c.model, c.datamodule)
    assert set(metrics) == {"val/l1", "val/fdl1", "val/sdl1", "val/mse", "val/loss"}
    assert all(math.isfinite(float(v)) for v in metrics.values()) and float(metrics["val/loss"]) > 0.0
    nc = c.datamodule._batcher.last_n_corners
    assert nc.shape == (125,) and bool((nc <= 12).all()) and int((nc >= 2).sum()) > 0

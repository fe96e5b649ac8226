"""GPU: the pair-alignment kernels (csrc/pair_align.hip, ``mod_extraction_amd.alignment``) against their definition in numpy
fp64 (tests/helpers/pair_align64.py), and the data path end to end on rendered pair files.

Gates, none of them measured on the kernels:
  r      |r - r64| <= N 2^-53 sum |dry wet| per entry: the bound of an fp64 sum of N exact products in any order (each of the
         at most N additions rounds a partial sum that never exceeds sum |dry wet| by 2^-53 relative).
  lag    equal, and the sign of corr equal, on every row: tests/test_pair_align64.py holds the table's peak at least 0.03 above
         the runner-up, eleven orders above what the order of an fp64 sum moves c by.
  corr   2^-23 relative: one fp32 rounding (2^-24) with the project's usual factor 2; the fp64 error before it is 1e-16.
  frac   2^-22 absolute, after asserting the helper's curvature |a - 2 b0 + c+| >= 0.05 on the rows: |frac| <= 0.5, so its
         fp32 rounding is at most 2^-25, and the fp64 differences of |c| (1e-15) over a curvature of 0.05 stay below 1e-13.
  shift  bit for bit.
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests.helpers import pair_align64 as h

pytestmark = pytest.mark.gpu
EPS53 = 2.0 ** -53
MIN_CURV = 0.05


@functools.lru_cache(maxsize=None)
def group(N, L):
    """The 20 table rows of one (N, L), stacked: (dry (20, N), wet (20, N), the helper's estimate of every row, the true
    (lag, pol) of every row).  Shared and not modified."""
    cases = [c for c in h.table() if (c[0], c[1]) == (N, L)]
    pairs = [h.make_pair(*c) for c in cases]
    dry, wet = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    return dry, wet, [h.estimate64(d, w, L) for d, w in pairs], [(c[3], c[4]) for c in cases]


def check_r(name, r_dev, ref, N):
    """Every entry against the derived bound; returns the worst |r - r64| / bound."""
    worst = 0.0
    for b, e in enumerate(ref):
        err = np.abs(r_dev[b] - e["r"])
        bound = N * EPS53 * e["s"]
        ratio = float(np.max(err / np.maximum(bound, 1e-300)))
        worst = max(worst, ratio)
        assert np.all(err <= bound), (name, b, ratio)
    print(f"{name}: worst |r - r64| / (N 2^-53 sum|dry wet|) = {worst:.3e}")
    return worst


@pytest.mark.parametrize("N,L", h.SIZES)
def test_xcorr_and_peak_against_the_helper(dev, N, L):
    from mod_extraction_amd import alignment as A
    dry, wet, ref, truth = group(N, L)
    d, w = torch.from_numpy(dry).to(dev), torch.from_numpy(wet).to(dev)
    r = A.xcorr_lags(d, w, L)
    assert r.shape == (len(ref), 2 * L + 1) and r.dtype == torch.float64
    check_r(f"N {N} L {L}", r.cpu().numpy(), ref, N)
    assert torch.equal(A.xcorr_lags(d, w, L), r)                              # a second launch: the same bits
    est = A.estimate_pair_lag(d, w, L)
    again = A.estimate_pair_lag(d, w, L)
    assert all(torch.equal(x, y) for x, y in zip(est, again))
    assert est.lag.dtype == torch.int32 and est.corr.dtype == est.frac.dtype == torch.float32
    lag, corr, frac = est.lag.cpu().numpy(), est.corr.cpu().numpy().astype(np.float64), est.frac.cpu().numpy().astype(np.float64)
    worst_c = worst_f = 0.0
    for b, e in enumerate(ref):
        assert (e["lag"], np.sign(e["corr"])) == truth[b]                     # the helper recovers the table (CPU test)
        assert lag[b] == e["lag"] and np.sign(corr[b]) == np.sign(e["corr"]), (b, lag[b], e["lag"])
        if abs(e["lag"]) == L:
            assert frac[b] == 0.0 and e["frac"] == 0.0                        # the window's edges
        else:
            assert abs(e["curv"]) >= MIN_CURV, (b, e["curv"])
        d_c = abs(corr[b] - e["corr"]) / abs(e["corr"])
        d_f = abs(frac[b] - e["frac"])
        worst_c, worst_f = max(worst_c, d_c), max(worst_f, d_f)
        tol = 2.0 ** -23
        assert d_c <= tol, (b, d_c)
        tol = 2.0 ** -22
        assert d_f <= tol, (b, d_f)
    print(f"N {N} L {L}: worst corr rel {worst_c:.3e} (gate {2.0 ** -23:.3e}), frac abs {worst_f:.3e} (gate {2.0 ** -22:.3e})")


def test_one_row_strided_rows_and_the_widest_window(dev):
    from mod_extraction_amd import alignment as A
    dry, wet, ref, _ = group(257, 8)
    # B = 1, as (N,) and as (1, 1, N)
    d1, w1 = torch.from_numpy(dry[3]).to(dev), torch.from_numpy(wet[3]).to(dev)
    r1 = A.xcorr_lags(d1, w1, 8)
    assert r1.shape == (1, 17) and torch.equal(A.xcorr_lags(d1.view(1, 1, -1), w1.view(1, 1, -1), 8), r1)
    check_r("B = 1", r1.cpu().numpy(), [ref[3]], 257)
    e1 = A.estimate_pair_lag(d1, w1, 8)
    assert e1.lag.shape == (1,) and int(e1.lag[0]) == ref[3]["lag"]
    # rows a row stride apart, read in place: dry and wet interleaved in one buffer, the gaps poisoned
    B = dry.shape[0]
    buf = torch.full((B, 2 * 257 + 7), float("nan"), device=dev)
    buf[:, 2:259] = torch.from_numpy(dry).to(dev)
    buf[:, 261:518] = torch.from_numpy(wet).to(dev)
    dv, wv = buf[:, 2:259], buf[:, 261:518]
    assert not dv.is_contiguous() and dv.stride(0) == 2 * 257 + 7
    dense = A.xcorr_lags(dv.contiguous(), wv.contiguous(), 8)
    rs = A.xcorr_lags(dv, wv, 8)
    check_r("strided", rs.cpu().numpy(), ref, 257)
    assert torch.equal(rs, dense)
    es, ed = A.estimate_pair_lag(dv, wv, 8), A.estimate_pair_lag(dv.contiguous(), wv.contiguous(), 8)
    assert all(torch.equal(x, y) for x, y in zip(es, ed)) and es.lag.cpu().tolist() == [e["lag"] for e in ref]
    # L = N - 1 at N = 300: every overlap down to one sample, four full lag tiles and a part of a tenth
    rng = np.random.default_rng(300)
    x = rng.standard_normal((3, 300)).astype(np.float32)
    y = np.roll(x, 5, axis=1) + 0.1 * rng.standard_normal((3, 300)).astype(np.float32)
    refw = [h.estimate64(x[b], y[b], 299) for b in range(3)]
    rw = A.xcorr_lags(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), 299)
    assert rw.shape == (3, 599)
    check_r("N 300 L 299", rw.cpu().numpy(), refw, 300)
    ew = A.estimate_pair_lag(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), 299)
    assert ew.lag.cpu().tolist() == [e["lag"] for e in refw] == [5, 5, 5]
    # L = 0: one lag, the window's edge
    e0 = A.estimate_pair_lag(torch.from_numpy(x).to(dev), torch.from_numpy(x).to(dev), 0)
    assert e0.lag.cpu().tolist() == [0, 0, 0] and e0.frac.cpu().tolist() == [0.0, 0.0, 0.0]
    assert np.allclose(e0.corr.cpu().numpy(), 1.0, rtol=0, atol=2.0 ** -23)


def test_silent_rows_and_ties_follow_the_rule(dev):
    from mod_extraction_amd import alignment as A
    rng = np.random.default_rng(9)
    x = rng.standard_normal(64).astype(np.float32)
    z = np.zeros(64, dtype=np.float32)
    ties = h.tie_rows(64)
    assert all(t[2] == 5 for t in ties)
    dry = np.stack([z, x, z, x] + [t[0] for t in ties])
    wet = np.stack([x, z, z, x] + [t[1] for t in ties])
    est = A.estimate_pair_lag(torch.from_numpy(dry).to(dev), torch.from_numpy(wet).to(dev), 5)
    lag, corr, frac = est.lag.cpu().tolist(), est.corr.cpu().tolist(), est.frac.cpu().tolist()
    assert lag[:3] == [0, 0, 0] and corr[:3] == [0.0, 0.0, 0.0] and frac[:3] == [0.0, 0.0, 0.0]
    assert lag[3] == 0 and abs(corr[3] - 1.0) <= 2.0 ** -23                  # a live row between them is untouched
    for k, (_, _, _, want, sign) in enumerate(ties):
        e = h.estimate64(dry[4 + k], wet[4 + k], 5)
        assert e["gap"] == 0.0 and e["lag"] == want
        assert lag[4 + k] == want and np.sign(corr[4 + k]) == sign, (k, lag[4 + k], corr[4 + k])
        assert abs(abs(corr[4 + k]) - 2.0 ** -0.5) <= 2.0 ** -23 * 2.0 ** -0.5


@pytest.mark.parametrize("N", [1, 5, 257, 4099])
def test_shift_is_the_numpy_restatement(dev, N):
    from mod_extraction_amd import alignment as A
    lags = sorted({0, 1, -1, N - 1, -(N - 1), 3, -6, 7, -2, 2, N, -(N + 3), N // 2 + 1, -(N // 3) - 2})
    B = len(lags)
    rng = np.random.default_rng(N)
    wet = rng.standard_normal((B, N)).astype(np.float32)
    corr = rng.standard_normal(B).astype(np.float32)
    corr[0], corr[1] = 0.0, -0.0                                              # not below zero: +1
    w, lag_t, corr_t = torch.from_numpy(wet).to(dev), torch.tensor(lags, dtype=torch.int32, device=dev), torch.from_numpy(corr).to(dev)
    plain = A.shift_rows(w, lag_t)
    assert plain.shape == (B, N) and torch.equal(plain.cpu(), torch.from_numpy(h.shift64(wet, lags)))
    signed = A.shift_rows(w, lag_t, corr_t)
    want = torch.from_numpy(h.shift64(wet, lags, corr))
    assert torch.equal(signed.cpu(), want)
    # into a strided out whose rows start at every alignment, a sentinel around them; the source strided as well
    big = torch.full((B + 2, N + 9), 777.0, device=dev)
    out = big[1:B + 1, 3:3 + N]
    src = torch.full((B, N + 5), float("nan"), device=dev)
    src[:, 1:1 + N] = w
    got = A.shift_rows(src[:, 1:1 + N], lag_t, corr_t, out=out)
    assert got is out and torch.equal(out.cpu(), want)
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[1:B + 1, 3:3 + N] = False
    assert bool((big[mask] == 777.0).all())
    # (B, 1, N) keeps its shape; (N,) is one row
    assert torch.equal(A.shift_rows(w.view(B, 1, N), lag_t, corr_t).cpu(), want.view(B, 1, N))
    assert torch.equal(A.shift_rows(w[2], lag_t[2:3]).cpu(), torch.from_numpy(h.shift64(wet[2:3], lags[2:3]))[0])


def test_align_pairs_lines_a_batch_up(dev):
    from mod_extraction_amd import alignment as A
    dry, wet, ref, truth = group(4096, 64)
    d, w = torch.from_numpy(dry).to(dev), torch.from_numpy(wet).to(dev)
    aligned, est = A.align_pairs(d, w, 64)
    assert est.lag.cpu().tolist() == [t[0] for t in truth]
    assert torch.equal(aligned.cpu(), torch.from_numpy(h.shift64(wet, est.lag.cpu().numpy(), est.corr.cpu().numpy())))
    again = A.estimate_pair_lag(d, aligned, 64)                               # aligned: lag 0 and positive on every row
    assert again.lag.cpu().tolist() == [0] * len(truth) and bool((again.corr > 0).all())


# ---- end to end: rendered pair files, the data module ---------------------------------------------------------------------
SR, NS, FRAMES = 44100, 8192, 5 * 8192
DELAYS = {"a.wav": (37, 1), "b.wav": (-12, -1), "c.wav": (0, 1)}


def delayed(y, d):
    """y late by d samples (early for d < 0), zeros where nothing is known: out[n] = y[n - d]."""
    out = torch.zeros_like(y)
    if d >= 0:
        out[d:] = y[:y.numel() - d]
    else:
        out[:d] = y[-d:]
    return out


@pytest.fixture(scope="module")
def pair_files(dev, tmp_path_factory):
    """dry / wet directories of four pairs: the wet is this package's flanger on the dry file, then late by 37 samples, early
    by 12 and inverted, as rendered; the fourth wet is unrelated noise.  Returns (dry_dir, wet_dir, {name: (dry, render)})."""
    from mod_extraction_amd import datasets as D, fx, modulations as M
    root = tmp_path_factory.mktemp("rendered")
    os.makedirs(root / "dry")
    os.makedirs(root / "wet")
    g = torch.Generator().manual_seed(20)
    flanger = fx.MonoFlangerChorusModule(1, 1, FRAMES, SR, max_min_delay_ms=1.0, max_lfo_delay_ms=10.0)
    files = {}
    for k, name in enumerate(list(DELAYS) + ["noise.wav"]):
        dry = 0.3 * torch.randn(FRAMES, generator=g)
        dry[:64] = 0.0                                      # so the render starts with zeros: reading before the file's
        mod = M.make_mod_signal(FRAMES, SR, 0.7 + 0.4 * k, phase=0.5 * k, shape="cos").to(dev)      # start is exact too
        y = flanger(dry.to(dev).view(1, 1, -1), mod.view(1, -1), feedback=0.3, min_delay_width=0.5, width=0.5, depth=0.8,
                    mix=0.4).view(-1).cpu()
        assert bool((y[:64] == 0.0).all())
        if name == "noise.wav":
            wet = 0.3 * torch.randn(FRAMES, generator=g)
        else:
            d, pol = DELAYS[name]
            wet = pol * delayed(y, d)
        D.wav_save(str(root / "dry" / name), dry.view(1, -1), SR)
        D.wav_save(str(root / "wet" / name), wet.view(1, -1), SR)
        files[name] = (dry.numpy(), y.numpy())
    return str(root / "dry"), str(root / "wet"), files


def module(pair_files, dev, **kw):
    from mod_extraction_amd import data_modules
    dm = data_modules.RandomAudioChunkDryWetDataModule(batch_size=8, n_samples=NS, sr=SR, dry_train_dir=pair_files[0],
                                                       wet_train_dir=pair_files[1], train_num_examples_per_epoch=8,
                                                       end_buffer_n_samples=64, **kw)
    dm.setup(dev)
    return dm


def locate(files, dry_chunk):
    c = dry_chunk.numpy()
    probe = c[100:104]                                       # past the zeroed start of a file
    for name, (dry, _) in files.items():
        for s in np.flatnonzero(dry[100:FRAMES - NS + 101] == probe[0]):
            if np.array_equal(dry[s:s + NS], c):
                return name, int(s)
    raise AssertionError("dry chunk not found")


def test_data_module_recovers_the_delays_and_reads_aligned_chunks(dev, pair_files):
    from mod_extraction_amd import datasets as D
    dm = module(pair_files, dev, align_max_lag_ms=5.0)
    table = dm.pair_alignment["train"]
    assert dm.pair_alignment["val"] is None and list(table) == ["a.wav", "b.wav", "c.wav", "noise.wav"]
    for name, al in table.items():
        print(name, al)
    for name, (lag, pol) in DELAYS.items():
        assert isinstance(table[name], D.PairAlignment)
        assert (table[name].lag, table[name].polarity, table[name].ok) == (lag, pol, True), (name, table[name])
        assert table[name].corr >= 0.5
    assert (table["noise.wav"].lag, table["noise.wav"].polarity, table["noise.wav"].ok) == (0, 1, False)
    assert table["noise.wav"].corr < 0.5
    plain = module(pair_files, dev)
    assert plain.pair_alignment == {"train": None, "val": None}
    seen, moved = set(), 0
    for k in range(3):
        torch.manual_seed(77 + k)
        dry, wet, mod_sig, params = dm.train_batch()
        torch.manual_seed(77 + k)
        dry_p, wet_p, _, _ = plain.train_batch()
        assert dry.shape == wet.shape == (8, 1, NS) and dry.is_cuda and mod_sig is None and params is None
        assert torch.equal(dry, dry_p)                                        # the same seeded stream of dry chunks
        for i in range(8):
            name, start = locate(pair_files[2], dry[i, 0].cpu())
            if name == "noise.wav":
                assert torch.equal(wet[i], wet_p[i])
                continue
            render = torch.from_numpy(pair_files[2][name][1][start:start + NS])
            assert torch.equal(wet[i, 0].cpu(), render), (name, start)        # the undelayed render at the same start
            if DELAYS[name] != (0, 1):
                assert not torch.equal(wet_p[i, 0].cpu(), render), (name, start)
                moved += 1
            seen.add(name)
    assert seen == set(DELAYS) and moved > 0

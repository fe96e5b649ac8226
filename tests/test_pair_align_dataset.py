"""CPU: the data path of the pair alignment -- ``datasets.RandomAudioChunkDryWetDataset`` with an alignment table installed
by ``set_alignment`` (no device), on a small float32 RIFF corpus: float32 files make every equality exact.  The wet file of
a pair holds a ramp that names its own sample index, so a chunk says where it was read."""
import logging
import os

import numpy as np
import pytest
import torch

from mod_extraction_amd import datasets as D

SR, N, FRAMES = 8000, 256, 3000
NAMES = ("a.wav", "b.wav", "c.wav")


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """dry/<name>: seeded noise; wet/<name>: 1 + index / 4096 + file number (exact in fp32, never zero)."""
    root = tmp_path_factory.mktemp("pairs")
    os.makedirs(root / "dry")
    os.makedirs(root / "wet")
    g = torch.Generator().manual_seed(3)
    files = {}
    for k, name in enumerate(NAMES):
        dry = 0.5 * torch.randn(1, FRAMES, generator=g)
        wet = (1.0 + torch.arange(FRAMES, dtype=torch.float32) / 4096.0 + k).view(1, -1)
        D.wav_save(str(root / "dry" / name), dry, SR)
        D.wav_save(str(root / "wet" / name), wet, SR)
        files[name] = (dry[0].numpy(), wet[0].numpy())
    return str(root / "dry"), str(root / "wet"), files


def make(corpus, **kw):
    return D.RandomAudioChunkDryWetDataset(corpus[0], corpus[1], N, SR, num_examples_per_epoch=16, check_dataset=False, **kw)


def items(ds, n, seed=17):
    torch.manual_seed(seed)                                                   # util.randint / util.choice draw from torch
    return [ds[i] for i in range(n)]


def locate(files, dry_chunk):
    """(file name, start) of a dry chunk: the corpus is noise, so the match is unique."""
    c = dry_chunk[0].numpy()
    for name, (dry, _) in files.items():
        hits = np.flatnonzero(dry[:FRAMES - N + 1] == c[0])
        for s in hits:
            if np.array_equal(dry[s:s + N], c):
                return name, int(s)
    raise AssertionError("dry chunk not found in the corpus")


def expected_wet(files, name, start, lag, pol):
    wet = files[name][1]
    idx = np.arange(start + lag, start + lag + N)
    inside = (idx >= 0) & (idx < FRAMES)
    out = np.zeros(N, dtype=np.float32)
    out[inside] = wet[idx[inside]]
    return np.float32(pol) * out, inside


def test_without_the_argument_items_are_the_parents(corpus):
    ds = make(corpus)
    assert ds.pair_alignment is None and ds.align_max_lag is None
    for dry, wet in items(ds, 12):
        name, start = locate(corpus[2], dry)
        assert np.array_equal(wet[0].numpy(), corpus[2][name][1][start:start + N])


def test_wet_is_read_at_start_plus_lag_times_polarity(corpus):
    table = {"a.wav": (37, 1), "b.wav": (-12, -1), "c.wav": (0, 1)}
    ds = make(corpus)
    ds.set_alignment(table)
    assert ds.pair_alignment["b.wav"] == D.PairAlignment(-12, -1, 1.0, True)
    seen = set()
    for dry, wet in items(ds, 40):
        name, start = locate(corpus[2], dry)
        lag, pol = table[name]
        want, _ = expected_wet(corpus[2], name, start, lag, pol)
        assert wet.shape == dry.shape == (1, N) and wet.dtype == torch.float32
        assert np.array_equal(wet[0].numpy(), want), (name, start)
        seen.add(name)
    assert seen == set(NAMES)


def test_the_dry_stream_of_a_seeded_run_does_not_move(corpus):
    plain, aligned = make(corpus), make(corpus, align_max_lag_ms=10.0)
    aligned.set_alignment({"a.wav": (37, 1), "b.wav": (-12, -1), "c.wav": (5, -1)})
    assert aligned.align_max_lag == 80
    a, b = items(plain, 20), items(aligned, 20)
    assert all(torch.equal(x[0], y[0]) for x, y in zip(a, b))
    assert not all(torch.equal(x[1], y[1]) for x, y in zip(a, b))
    assert aligned.probe_starts(aligned.dry_paths[0]) == aligned.probe_starts(aligned.dry_paths[0])       # no draw
    c = items(plain, 20)
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, c))                 # seeded: repeatable


def test_zeros_exactly_where_the_index_leaves_the_file(corpus, monkeypatch):
    ds = make(corpus)
    name = "a.wav"
    path = [p for p in ds.dry_paths if p.endswith(name)][0]
    for start, lag in ((0, -12), (FRAMES - N, 37), (5, -5), (FRAMES - N - 37, 37), (100, 4000), (100, -4000)):
        ds.set_alignment({name: (lag, -1)})
        chunk = D.wav_load(path, frame_offset=start, num_frames=N)[0]
        monkeypatch.setattr(ds, "search_dataset_for_audio_chunk", lambda n, e, c=chunk, s=start: (c, path, 0, s))
        dry, wet = ds[0]
        want, inside = expected_wet(corpus[2], name, start, lag, -1)
        assert torch.equal(dry, chunk) and np.array_equal(wet[0].numpy(), want)
        assert np.array_equal(wet[0].numpy() == 0.0, ~inside)                 # the ramp is never zero inside the file
        assert int((~inside).sum()) == min(N, max(0, -(start + lag)) + max(0, start + lag + N - FRAMES))


def test_end_buffer_keeps_positive_lags_inside(corpus):
    ds = make(corpus, end_buffer_n_samples=37)
    ds.set_alignment({n: (37, 1) for n in NAMES})
    for dry, wet in items(ds, 40):
        assert bool((wet != 0.0).all())


def test_set_alignment_checks_and_removal(corpus):
    ds = make(corpus)
    with pytest.raises(ValueError, match="no pair named"):
        ds.set_alignment({"z.wav": (1, 1)})
    with pytest.raises(ValueError, match="polarity"):
        ds.set_alignment({"a.wav": (1, 0)})
    ds.set_alignment({"a.wav": D.PairAlignment(3, -1, 0.8, True)})
    assert ds.pair_alignment == {"a.wav": D.PairAlignment(3, -1, 0.8, True)}
    ds.set_alignment(None)
    assert ds.pair_alignment is None
    with pytest.raises(ValueError, match="align_max_lag_ms"):
        ds.estimate_alignment(torch.device("cpu"))
    for bad in (0.0, -1.0, 2000.0, 40.0):                                      # 40 ms = 320 samples > n_samples - 1
        with pytest.raises(ValueError, match="align_max_lag_ms"):
            make(corpus, align_max_lag_ms=bad)
    with pytest.raises(ValueError, match="align_n_probes"):
        make(corpus, align_max_lag_ms=10.0, align_n_probes=0)


def test_probe_starts_are_evenly_spaced_and_deterministic(corpus):
    ds = make(corpus, align_max_lag_ms=10.0, align_n_probes=8)
    span = FRAMES - N
    assert ds.probe_starts(ds.dry_paths[0]) == [(span * k) // 7 for k in range(8)]
    assert make(corpus, align_max_lag_ms=10.0, align_n_probes=1).probe_starts(ds.dry_paths[0]) == [span // 2]
    assert make(corpus, align_max_lag_ms=10.0, align_n_probes=2).probe_starts(ds.dry_paths[0]) == [0, span]


def test_reduction_rules():
    """Median, polarity and flag of the per-file reduction, on fed-in probe results."""
    R = D.reduce_probe_lags
    assert R([37, 37, 37], [0.9, 0.8, 0.7], 0.5) == D.PairAlignment(37, 1, pytest.approx(0.8), True)
    assert R([37, 137, 37, -63, 37], [0.9, 0.8, 0.9, 0.7, 0.9], 0.5).lag == 37           # outliers a period off are outvoted
    assert R([5, 3, 9, 7], [0.9] * 4, 0.5).lag == 5                                        # the LOWER median of an even count
    assert R([4], [-0.6], 0.5) == D.PairAlignment(4, -1, pytest.approx(0.6), True)
    assert R([-12, -12, -12], [-0.9, 0.2, -0.8], 0.5).polarity == -1                       # the summed corr decides
    assert R([2, 2], [0.7, -0.7], 0.5).polarity == 1                                       # a zero sum is +1
    low = R([37, 37, 12], [0.4, 0.45, 0.9], 0.5)
    assert low == D.PairAlignment(0, 1, pytest.approx(0.45), False)                        # median |corr| below the gate
    assert R([37, 37, 12], [0.4, 0.5, 0.9], 0.5).ok and R([1], [0.5], 0.5).ok              # at the gate is trusted
    assert R([], [], 0.5) == D.PairAlignment(0, 1, 0.0, False)
    assert R([3], [float("nan")], 0.5) == D.PairAlignment(0, 1, pytest.approx(float("nan"), nan_ok=True), False)
    with pytest.raises(ValueError):
        R([1, 2], [0.5], 0.5)


def test_estimate_reduces_per_file_and_warns(corpus, monkeypatch, caplog):
    """``estimate_alignment`` with the device call replaced by a table of probe results: files are stacked up to the row
    budget, reduced one by one, the untrusted one is named in one warning, and silent probes are left out."""
    from mod_extraction_amd import alignment as A
    ds = make(corpus, align_max_lag_ms=10.0, align_n_probes=4)
    monkeypatch.setattr(ds, "ALIGN_ROW_BUDGET", 8)
    calls = []

    def fake(dry, wet, max_lag):
        assert dry.shape == wet.shape and dry.size(1) == N and max_lag == 80 and dry.size(0) <= 8
        calls.append(dry.size(0))
        which = [int(float(w[0]) - 1.0) for w in wet]                         # the file number rides on the ramp (ramp < 1)
        lag = torch.tensor([(37, -12, 5)[k] for k in which], dtype=torch.int32)
        corr = torch.tensor([(0.9, -0.8, 0.1)[k] for k in which])
        return A.PairLag(lag, torch.zeros(len(which)), corr)

    monkeypatch.setattr(A, "estimate_pair_lag", fake)
    with caplog.at_level(logging.WARNING, logger=D.__name__):
        table = ds.estimate_alignment(torch.device("cpu"))
    assert calls == [8, 4]                                                    # two files fit the budget of 8 rows, then one
    assert list(table) == list(NAMES) and ds.pair_alignment is table
    assert table["a.wav"] == D.PairAlignment(37, 1, pytest.approx(0.9), True)
    assert table["b.wav"] == D.PairAlignment(-12, -1, pytest.approx(0.8), True)
    assert table["c.wav"] == D.PairAlignment(0, 1, pytest.approx(0.1), False)
    warned = [r for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warned) == 1 and "c.wav" in warned[0].getMessage() and "a.wav" not in warned[0].getMessage()
    # every probe silent: no call at all, every file flagged
    calls.clear()
    quiet = make(corpus, align_max_lag_ms=10.0, silence_threshold_energy=10.0)
    assert all(not al.ok and al.lag == 0 for al in quiet.estimate_alignment(torch.device("cpu")).values()) and calls == []

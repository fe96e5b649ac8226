"""GPU: recordings at 48 kHz reach a 44.1 kHz data module (K24).  Three dry / wet wav pairs of 1.5 s at 48 kHz -- each dry a
sum of sines below 15 kHz, each wet the same delayed by 37 samples -- are dropped by the pair dataset as they lie on disk (it
then has no file and raises, as it always has); with ``resample_cache_dir`` the data module converts them on the device at
``setup`` and hands out batches.  Every converted file is checked against the fp64 restatement on the file's own samples (the
rows gate of tests/test_gpu_resample.py) and, away from its two ends, against the sines it samples:

    |y - analytic| <= 1e-6: the sum has amplitude <= 0.75, so the fp32 roundings of the input (2^-25 each, through a filter of
    unit gain) and of the output stay below 1e-7, and the restatement's own error on such sines is 1.5e-8
    (tests/test_resample64.py).

A second ``setup`` converts nothing (no file of the cache is touched), and scripts/resample_dir.py, run as a fresh child
process, writes the same bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import resample64 as h

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR_IN, SR, L, DELAY, N_SAMPLES = 48000, 44100, 72000, 37, 8192
NAMES = ("take_a.wav", "take_b.wav", "take_c.wav")


def tones(seed):
    r = np.random.default_rng(seed)
    return [(float(f), 0.25, float(ph)) for f, ph in zip(r.uniform(80.0, 15000.0, 3), r.uniform(0.0, 2 * np.pi, 3))]


def sines(seed, t):
    """The pair's dry signal at the times t (seconds), fp64."""
    return sum(a * np.sin(2 * np.pi * f * t + ph) for f, a, ph in tones(seed))


@pytest.fixture(scope="module")
def raw(tmp_path_factory):
    from scipy.io import wavfile
    root = tmp_path_factory.mktemp("pairs48k")
    t = np.arange(L) / SR_IN
    for seed, name in enumerate(NAMES):
        dry = sines(seed, t).astype(np.float32)
        wet = np.concatenate([np.zeros(DELAY, dtype=np.float32), dry[:L - DELAY]])
        for which, a in (("dry", dry), ("wet", wet)):
            os.makedirs(root / which, exist_ok=True)
            wavfile.write(str(root / which / name), SR_IN, a)
    return root


def tree(d):
    return sorted(os.path.relpath(os.path.join(p, f), d) for p, _, fs in os.walk(d) for f in fs)


def test_the_raw_directories_hold_nothing_for_a_44100_dataset(raw):
    from mod_extraction_amd import datasets
    with pytest.raises(AssertionError):
        datasets.RandomAudioChunkDryWetDataset(str(raw / "dry"), str(raw / "wet"), N_SAMPLES, SR)


def test_the_data_module_converts_reads_and_caches(dev, raw, tmp_path):
    from mod_extraction_amd import data_modules, datasets, resample
    cache = tmp_path / "cache"
    dm = data_modules.RandomAudioChunkDryWetDataModule(
        batch_size=4, n_samples=N_SAMPLES, sr=SR, train_num_examples_per_epoch=8, val_num_examples_per_epoch=4,
        dry_train_dir=str(raw / "dry"), wet_train_dir=str(raw / "wet"), resample_cache_dir=str(cache))
    dm.setup(dev)
    for batch in (dm.train_batch(), dm.val_batch()):
        dry, wet, mod, params = batch
        assert mod is None and params is None and dry.shape == wet.shape == (4, 1, N_SAMPLES) and dry.device == dev
        assert float(dry.abs().max()) > 0.1 and float(wet.abs().max()) > 0.1 and float(dry.abs().max()) <= 0.76
    assert sorted(os.listdir(cache)) == ["dry_train", "wet_train"]
    stamps = [n + resample.STAMP_SUFFIX for n in NAMES]
    assert tree(cache / "dry_train") == tree(cache / "wet_train") == sorted(NAMES + tuple(stamps))

    # every converted file: its length, the restatement on the file's samples, the sines it samples
    pl = resample.resample_plan(SR_IN, SR)
    hp = h.plan(SR_IN, SR)
    table = pl.taps(dev).cpu().numpy()
    n_out = -(-L * 147 // 160)
    m = np.arange(n_out)
    inner = slice(200, n_out - 200)
    for seed, name in enumerate(NAMES):
        for which, delay in (("dry", 0), ("wet", DELAY)):
            src, sr_src = datasets.wav_load(str(raw / which / name))
            got, sr_got = datasets.wav_load(str(cache / f"{which}_train" / name))
            assert (sr_src, sr_got) == (SR_IN, SR) and got.shape == (1, n_out) == (1, pl.out_length(L))
            y = got.numpy()[0].astype(np.float64)
            y64, bound = h.rows(src.numpy()[0], hp, table=table, with_bound=True)
            tol = 2.0 ** -24 * np.abs(y64) + hp.taps_per_phase * 2.0 ** -53 * bound
            assert float((np.abs(y - y64) - tol).max()) <= 0.0, (name, which)
            err = float(np.abs(y - sines(seed, m / SR - delay / SR_IN))[inner].max())
            print(f"{which}/{name}: interior |y - analytic| = {err:.2e}")
            assert err <= 1e-6
            stamp = json.load(open(str(cache / f"{which}_train" / name) + resample.STAMP_SUFFIX))
            assert (stamp["sr_in"], stamp["sr"], stamp["frames_in"], stamp["frames_out"]) == (SR_IN, SR, L, n_out)

    # a second setup converts nothing: no file of the cache, stamps included, is written again
    files = [str(cache / d / f) for d in ("dry_train", "wet_train") for f in tree(cache / d)]
    before = {f: (os.stat(f).st_mtime_ns, os.stat(f).st_ino) for f in files}
    dm2 = data_modules.RandomAudioChunkDryWetDataModule(
        batch_size=4, n_samples=N_SAMPLES, sr=SR, train_num_examples_per_epoch=8, val_num_examples_per_epoch=4,
        dry_train_dir=str(raw / "dry"), wet_train_dir=str(raw / "wet"), resample_cache_dir=str(cache))
    dm2.setup(dev)
    assert {f: (os.stat(f).st_mtime_ns, os.stat(f).st_ino) for f in files} == before
    assert dm2.train_batch()[0].shape == (4, 1, N_SAMPLES)

    # the command-line tool, as a fresh process: the same bytes
    out = tmp_path / "by_script"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "resample_dir.py"), "--in_dir", str(raw / "wet"),
                        "--out_dir", str(out), "--sr", str(SR), "--device", str(dev)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert rows == [{"file": n, "sr_in": SR_IN, "sr_out": SR, "frames_in": L, "frames_out": n_out} for n in NAMES]
    for name in NAMES:
        assert open(out / name, "rb").read() == open(cache / "wet_train" / name, "rb").read(), name


def test_without_the_key_nothing_is_converted(dev, raw, tmp_path, monkeypatch):
    from mod_extraction_amd import data_modules, resample
    monkeypatch.setattr(resample, "convert_tree", lambda *a, **k: pytest.fail("convert_tree without resample_cache_dir"))
    dm = data_modules.RandomAudioChunkDryWetDataModule(batch_size=2, n_samples=N_SAMPLES, sr=SR, dry_train_dir=str(raw / "dry"),
                                                       wet_train_dir=str(raw / "wet"))
    with pytest.raises(AssertionError):                          # the parent's behaviour: no file at 44.1 kHz
        dm.setup(dev)

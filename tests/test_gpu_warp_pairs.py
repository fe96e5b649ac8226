"""GPU: recorded pairs on two clocks (K26) end to end -- the estimate, the cache on disk, the data module, ``score_pair`` and
the two scripts -- on the pairs of tests/helpers/warp64.py, whose own figures tests/test_warp64.py gates (ESR of
estimate-then-warp 7.3e-6 / 2.7e-6, of the constant lag 0.37 / 0.27).  ALL FAIL WITHOUT THE FEATURE.

The files (3 s at 44.1 kHz, float32, written once to a temporary directory): ``p300`` (+300 ppm, +37.4 samples, its wet 40
frames longer than its dry), ``m120`` (-120 ppm, -12.3 samples, inverted), ``late5`` (late by exactly 5 samples, one clock)
and ``other`` (an unrelated wet).  The four dry files are ONE signal at the gains 1, 1/2, 1/4, 1/8 -- exact in fp32, the
effect is linear below its clip -- so that a batch item names its file by its level.

ESR gates are like for like: a batch item against the undrifted render at its dry chunk's position may have 1.5 times the
ESR of the HELPER's warped wet on the same samples, + 1e-7: the margin covers the fp32 rounding of the warped file and the
1e-6 samples between the two lines, and nothing else differs.  Samples within ``TRIM`` of a file's ends are left out on both
sides: there the recording does not hold what the line asks for.

Measured on the MI355X (profiles/r28/README.md): the device's line is the helper's to 8.1e-9 samples and 8.6e-14 in drift; the
warped files have the helper's ESR to the printed digit (7.350e-6, 2.711e-6); K19 alone leaves batch ESRs of 0.32 .. 0.34;
``score_pair`` along the line 9.012e-5 against the fp64 helper's 9.012e-5, without ``drift`` 0.632."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import flanger_adjoint64 as fa
from tests.helpers import lfo_stitch64 as S
from tests.helpers import warp64 as h
from tests.helpers.flanger_adjoint64_lr import upsample64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR, L = h.SR, h.L
GAINS = {"p300": 1.0, "m120": 0.5, "late5": 0.25, "other": 0.125}
LAG_MS = 128 / 44.1                                              # 128 samples: h.MAX_LAG
N = 32768                                                        # the data module's chunk


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{"root", "dry", "wet"}: the raw directories, written once and left unchanged."""
    from scipy.io import wavfile
    root = tmp_path_factory.mktemp("pairs")
    dry, wet = h.source()
    wet32 = wet.astype(np.float32)
    late = np.concatenate([np.zeros(5, np.float32), wet32[:L - 5]])
    unrelated = (0.1 * np.random.default_rng(77).standard_normal(L)).astype(np.float32)
    wets = {"p300": h.recorded("p300"), "m120": h.recorded("m120"), "late5": late, "other": unrelated}
    for d in ("dry", "wet"):
        os.makedirs(root / d)
    for name, g in GAINS.items():
        wavfile.write(str(root / "dry" / f"{name}.wav"), SR, np.float32(g) * dry)
        wavfile.write(str(root / "wet" / f"{name}.wav"), SR, np.float32(g) * wets[name])
    return {"root": root, "dry": str(root / "dry"), "wet": str(root / "wet"), "late": late}


def tree(files, dev, name="cache"):
    from mod_extraction_amd import alignment
    return alignment.warp_tree(files["dry"], files["wet"], str(files["root"] / name), SR, h.MAX_LAG, device=dev,
                               probe_points=h.PROBE, n_probes=h.N_PROBES)


def esr_of(a, b, lo, hi):
    """ESR of a against b (chunks that start at file sample ``lo``) over the samples at least TRIM from the file's ends."""
    keep = slice(max(0, h.TRIM - lo), len(b) - max(0, hi - (L - h.TRIM)))
    a, b = np.asarray(a, np.float64)[keep], np.asarray(b, np.float64)[keep]
    return float(((a - b) ** 2).sum() / (b ** 2).sum())


@pytest.mark.parametrize("name", sorted(h.PAIRS))
def test_estimate_file_drift_is_the_helpers(dev, name):
    from mod_extraction_amd import alignment
    dry, _ = h.source()
    rec = h.recorded(name)
    want = h.acceptance(name)
    c, lags, fracs, corrs = want["probes"]
    d, w = torch.from_numpy(np.array(dry)).to(dev), torch.from_numpy(np.array(rec)).to(dev)
    hop, _ = alignment.probe_starts(L, len(rec), h.PROBE, h.N_PROBES)
    assert hop >= h.PROBE                                        # the strided views, no copy
    est = alignment.estimate_pair_lag(d.as_strided((h.N_PROBES, h.PROBE), (hop, 1)), w.as_strided((h.N_PROBES, h.PROBE), (hop, 1)),
                                      h.MAX_LAG)
    assert est.lag.cpu().tolist() == lags.astype(int).tolist()                # the helper's probe lags exactly
    assert float(np.abs(est.frac.cpu().numpy() - fracs).max()) <= 1e-5 and float(np.abs(est.corr.cpu().numpy() - corrs).max()) <= 1e-5
    got = alignment.estimate_file_drift(d, w, h.MAX_LAG, h.PROBE, h.N_PROBES)
    line = want["line"]
    print(f"{name}: device line {got.offset:.6f} + {1e6 * got.drift:.4f} ppm, helper {line.offset:.6f} + {1e6 * line.drift:.4f} ppm")
    assert got.ok and got.polarity == line.polarity == h.PAIRS[name][2] and got.n_probes == h.N_PROBES
    assert abs(got.offset - line.offset) <= 1e-6
    assert abs(got.drift - line.drift) <= 1e-9
    assert abs(got.resid - line.resid) <= 1e-5 and abs(got.corr - line.corr) <= 1e-5
    # probes that overlap (a gathered copy instead of views) see the same file
    short = alignment.estimate_file_drift(d[:40000], w[:40000], h.MAX_LAG, h.PROBE, 9)
    assert short.ok and abs(short.drift - h.PAIRS[name][0]) <= 2e-5


def test_warp_tree_and_align_dir(dev, files):
    from scipy.io import wavfile
    from mod_extraction_amd import alignment
    table = tree(files, dev)
    cache = files["root"] / "cache"
    assert sorted(table) == ["late5.wav", "m120.wav", "other.wav", "p300.wav"]
    stamps = {n: json.load(open(cache / f"{n}.wav.warped.json")) for n in GAINS}
    assert {n: s["route"] for n, s in stamps.items()} == {"p300": "warp", "m120": "warp", "late5": "shift", "other": "copy"}
    for name, (drift, offset, pol, _) in h.PAIRS.items():
        p = table[f"{name}.wav"]
        assert p.ok and p.polarity == pol and abs(1e6 * (p.drift - drift)) <= 1.0 and abs(p.offset - offset) <= 0.05
        sr, y = wavfile.read(str(cache / f"{name}.wav"))
        assert sr == SR and y.dtype == np.float32 and y.shape == (L,)                       # the DRY's frame count
        want = h.acceptance(name)
        got, ref = esr_of(y / GAINS[name], h.source()[1], 0, L), want["esr"]
        print(f"{name}: ESR of the warped file against the true wet {got:.3e}; the helper's {ref:.3e}")
        assert got <= 1.5 * ref + 1e-7
    # one clock: the integer path, the wet's own samples bit for bit
    late = table["late5.wav"]
    assert late.ok and late.polarity == 1 and round(late.offset) == 5 and abs(late.drift) * L < 0.25
    y = wavfile.read(str(cache / "late5.wav"))[1]
    want = np.concatenate([files["late"][5:], np.zeros(5, np.float32)]) * np.float32(GAINS["late5"])
    assert y.dtype == np.float32 and np.array_equal(y, want)
    # untrusted: flagged, copied byte for byte
    assert not table["other.wav"].ok and (table["other.wav"].offset, table["other.wav"].drift, table["other.wav"].polarity) == (0.0, 0.0, 1)
    assert open(cache / "other.wav", "rb").read() == open(os.path.join(files["wet"], "other.wav"), "rb").read()
    # a second run touches no file and returns the same table
    before = {f: os.stat(cache / f).st_mtime_ns for f in sorted(os.listdir(cache))}
    assert len(before) == 8 and tree(files, dev) == table
    assert {f: os.stat(cache / f).st_mtime_ns for f in sorted(os.listdir(cache))} == before
    # the shell form, as a child process: the same bytes
    out = files["root"] / "by_script"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "align_dir.py"), "--dry_dir", files["dry"], "--wet_dir", files["wet"],
                          "--out_dir", str(out), "--sr", str(SR), "--max_lag_ms", str(LAG_MS), "--probe_points", str(h.PROBE),
                          "--n_probes", str(h.N_PROBES), "--device", str(dev)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rows = {r["file"]: r for r in (json.loads(l) for l in run.stdout.splitlines() if l.startswith("{"))}
    assert sorted(rows) == sorted(table) and all(rows[f]["ok"] == table[f].ok and rows[f]["offset"] == table[f].offset for f in table)
    for name in GAINS:
        assert open(out / f"{name}.wav", "rb").read() == open(cache / f"{name}.wav", "rb").read(), name


def module(files, dev, **kw):
    from mod_extraction_amd import data_modules
    dm = data_modules.RandomAudioChunkDryWetDataModule(batch_size=8, n_samples=N, sr=SR, check_dataset=False, align_max_lag_ms=LAG_MS,
                                                       align_n_probes=4, end_buffer_n_samples=16, **kw)
    dm.setup(dev)
    return dm


def items(dm, n_batches):
    """(file name, start, dry, wet) of every item of ``n_batches`` training batches, by the dry chunk's level and head."""
    dry_file = h.source()[0]
    heads = np.lib.stride_tricks.sliding_window_view(dry_file, 16)
    out = []
    for _ in range(n_batches):
        dry, wet, _, _ = dm.train_batch()
        assert dry.shape == wet.shape == (8, 1, N) and dry.is_cuda and wet.is_cuda
        for d, w in zip(dry[:, 0].cpu().numpy(), wet[:, 0].cpu().numpy()):
            for name, g in GAINS.items():
                hit = np.nonzero((heads == d[:16] / np.float32(g)).all(1))[0]
                if hit.size:
                    out.append((name, int(hit[0]), d, w / g))
                    break
            else:
                raise AssertionError("a dry chunk that is in no file")
    return out


def test_data_module_on_the_cache(dev, files):
    _, true = h.source()
    # K19 alone on the raw directories: the pair whose wet is 40 frames longer is dropped (end_buffer_n_samples = 16 < 40)
    raw = module(files, dev, dry_train_dir=files["dry"], wet_train_dir=files["wet"])
    assert sorted(os.path.basename(p) for p in raw._pairs["train"].dry_paths) == ["late5.wav", "m120.wav", "other.wav"]
    assert raw.pair_drift == {"train": None, "val": None}
    dm = module(files, dev, dry_train_dir=files["dry"], wet_train_dir=files["wet"], align_drift_cache_dir=str(files["root"] / "dm_cache"),
                align_drift_n_probes=h.N_PROBES, align_drift_probe_ms=1e3 * h.PROBE / SR)       # the helper's probes: the same line
    ds = dm._pairs["train"]
    assert ds.wet_dir == str(files["root"] / "dm_cache" / "wet_train") and len(ds.dry_paths) == 4
    drift = dm.pair_drift["train"]
    assert sorted(drift) == sorted(f"{n}.wav" for n in GAINS) and not drift["other.wav"].ok
    # the datasets' own K19 estimate still runs, and finds nothing left to do on a trusted pair
    al = dm.pair_alignment["train"]
    for name in ("p300", "m120", "late5"):
        assert drift[f"{name}.wav"].ok and (al[f"{name}.wav"].lag, al[f"{name}.wav"].polarity, al[f"{name}.wav"].ok) == (0, 1, True)
    seen, worst = set(), 0.0
    for name, s, d, w in items(dm, 6):
        if name == "other":
            continue
        seen.add(name)
        got = esr_of(w, true[s:s + N], s, s + N)
        ref = 0.0 if name == "late5" else esr_of(h.acceptance(name)["warped"][s:s + N], true[s:s + N], s, s + N)
        worst = max(worst, got / (1.5 * ref + 1e-7))
        assert got <= 1.5 * ref + 1e-7, (name, s, got, ref)
    print(f"batches from the cache: worst ESR / gate {worst:.3f} over {sorted(seen)}")
    assert seen == {"p300", "m120", "late5"}


def test_k19_alone_on_the_drifted_pairs(dev, files):
    """The parent's path on equal-length copies of the two drifted pairs: one constant lag a file leaves an ESR of 0.1 and
    more on a batch (the helper's whole-file figures are 0.37 and 0.27)."""
    from scipy.io import wavfile
    _, true = h.source()
    root = files["root"] / "equal"
    for d in ("dry", "wet"):
        os.makedirs(root / d, exist_ok=True)
    for name in h.PAIRS:
        for d in ("dry", "wet"):
            sr, a = wavfile.read(os.path.join(files[d], f"{name}.wav"))
            wavfile.write(str(root / d / f"{name}.wav"), sr, a[:L])
    dm = module(files, dev, dry_train_dir=str(root / "dry"), wet_train_dir=str(root / "wet"))
    al = dm.pair_alignment["train"]
    assert all(v.ok for v in al.values()) and al["m120.wav"].polarity == -1
    for b in range(3):
        num = den = 0.0
        for name, s, d, w in items(dm, 1):
            keep = slice(max(0, h.TRIM - s), N - max(0, s + N - (L - h.TRIM)))
            t = true[s:s + N][keep]
            num, den = num + float(((w.astype(np.float64)[keep] - t) ** 2).sum()), den + float((t ** 2).sum())
        print(f"K19 alone, batch {b}: ESR {num / den:.3f}")
        assert num / den >= 0.1


class Stub(torch.nn.Module):
    """Returns the true LFO of every window it is shown, found in ``wet_file`` by the window's first 16 samples."""
    N_F = 345

    def __init__(self, wet_file, n):
        super().__init__()
        self.heads, self.n = wet_file.unfold(0, 16, 1), n

    def forward(self, x):
        lfos = []
        for row in x[:, -1, :]:
            s = int((self.heads == row[:16]).all(1).nonzero()[0, 0])
            p = s + np.arange(self.N_F) * (self.n - 1) / (self.N_F - 1)
            lfos.append((0.5 + 0.45 * np.sin(2.0 * np.pi * 0.7 * p / SR + 0.3)).astype(np.float32))
        return torch.from_numpy(np.stack(lfos)).to(x.device).unsqueeze(1), torch.zeros(x.size(0), 4, 8, device=x.device)


def rows_esr(a, b, n):
    """effect_losses' esr: the mean over consecutive rows of n samples of sum (a - b)^2 / (sum b^2 + 1e-8)"""
    a, b = np.asarray(a, np.float64)[:len(a) // n * n].reshape(-1, n), np.asarray(b, np.float64)[:len(b) // n * n].reshape(-1, n)
    return float((((a - b) ** 2).sum(1) / ((b ** 2).sum(1) + 1e-8)).mean())


def test_score_pair_along_the_line(dev):
    from mod_extraction_amd import alignment, lightning
    from mod_extraction_amd.file_eval import score_pair
    name, n = "p300", SR
    dry, _ = h.source()
    rec = h.recorded(name)
    d, w = torch.from_numpy(np.array(dry)).to(dev), torch.from_numpy(np.array(rec)).to(dev)
    step = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect="flanger", audio_loss_dict={"esr": 1.0})
    assert step.max_delay_samples == h.M_DELAY
    consts = {k: v.cpu().numpy() for k, v in step.clip_constants(h.FX_PARAMS, 1, dev).items()}
    assert all(np.array_equal(consts[k], v) for k, v in h.flanger_consts().items())          # the helper's effect is the step's
    est = alignment.estimate_file_drift(d, w, h.MAX_LAG, h.PROBE, h.N_PROBES)
    warped = alignment.warp_rows(w, est.offset, est.drift, n_out=L, polarity=est.polarity)
    out = score_pair(step, Stub(warped, n), d, w, n_samples=n, fx_params=h.FX_PARAMS, drift=est)
    assert out["drift_ppm"] == 1e6 * est.drift and out["lag_offset"] == est.offset and out["wet_hat"].shape == (L,)
    pair = score_pair(step, Stub(warped, n), d, w, n_samples=n, fx_params=h.FX_PARAMS, drift=(est.offset, est.drift))
    assert float(pair["esr"]) == float(out["esr"])
    # fp64: the helper's re-render from the fp64 track, scored against the helper-warped wet
    track64, _ = S.stitch(np.stack(true_windows(n)), window_starts(n), L, n, out["track"].numel())
    hat64 = fa.forward(np.array(dry)[None, :], upsample64(track64[None, :], L).astype(np.float32), h.flanger_consts(), h.M_DELAY)["y"][0]
    want = rows_esr(hat64, h.acceptance(name)["warped"], n)
    got = float(out["esr"])
    plain = score_pair(step, Stub(w[:L], n), d, w[:L], n_samples=n, fx_params=h.FX_PARAMS)
    assert "drift_ppm" not in plain and "lag_offset" not in plain
    print(f"score_pair along the line: esr {got:.3e}; the fp64 helper's {want:.3e}; without drift {float(plain['esr']):.3e}")
    assert got <= 1.5 * want + 1e-7
    assert float(plain["esr"]) >= 100.0 * got
    with pytest.raises(ValueError, match="beside drift"):
        score_pair(step, None, d, w, lag=3, drift=(0.0, 1e-4))
    with pytest.raises(ValueError, match="must be trusted"):
        score_pair(step, None, d, w, drift=alignment.PairDrift(0.0, 0.0, 1, 0.1, 0.0, 0, False))
    with pytest.raises(ValueError, match="PairDrift or"):
        score_pair(step, None, d, w, drift=3.0)
    with pytest.raises(ValueError, match="same length"):
        score_pair(step, None, d, w)


def window_starts(n):
    from mod_extraction_amd.file_eval import window_starts as ws
    return ws(L, n)


def true_windows(n):
    """What the stub returns for the windows of ``window_starts``, in their order: the true LFO at each window's points, fp32."""
    p = np.arange(Stub.N_F) * (n - 1) / (Stub.N_F - 1)
    return [(0.5 + 0.45 * np.sin(2.0 * np.pi * 0.7 * (s + p) / SR + 0.3)).astype(np.float32) for s in window_starts(n)]


CONFIG = """
data:
  class_path: mod_extraction.data_modules.RandomAudioChunkDryWetDataModule
  init_args: {{batch_size: 4, n_samples: 22272, sr: {sr}, align_max_lag_ms: {ms}, align_n_probes: 3, align_min_corr: 0.3,
              end_buffer_n_samples: 64}}
model:
  class_path: mod_extraction.lightning.LFOExtractionThroughEffect
  init_args:
    model: {model}
    sr: {sr}
    effect: flanger
    audio_loss_dict: {{esr: 1.0}}
    learned_fx:
      flanger:
        feedback: {{min: 0.0, max: 0.95, init: 0.3}}
        depth: 1.0
        mix: 0.5
        width: 0.9
        min_delay_width: 1.0
"""


def test_eval_pairs_with_drift_as_a_child(dev, files, tmp_path):
    from mod_extraction_amd import cli
    cfg_path = tmp_path / "eval.yml"
    cfg_path.write_text(CONFIG.format(sr=SR, ms=LAG_MS, model=os.path.join(ROOT, "configs", "models", "spectral_2dcnn.yml")))
    torch.manual_seed(5)
    step = cli.instantiate(cli.apply_links(cli.load_config(str(cfg_path)))["model"])
    ckpt = tmp_path / "fresh.ckpt"
    torch.save({"state_dict": step.state_dict()}, str(ckpt))
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "eval_pairs.py"), "-c", str(cfg_path), "--ckpt", str(ckpt), "--dry_dir", files["dry"],
           "--wet_dir", files["wet"], "--batch_size", "4", "--device", str(dev), "--drift", "--drift_n_probes", str(h.N_PROBES)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    by = {r["file"]: r for r in (json.loads(l) for l in run.stdout.splitlines() if l.startswith("{"))}
    print({f: {k: r.get(k) for k in ("drift_ppm", "lag_offset", "drift_resid", "drift_ok", "esr")} for f, r in by.items()})
    assert sorted(by) == ["late5.wav", "m120.wav", "other.wav", "p300.wav"]
    assert abs(by["p300.wav"]["drift_ppm"] - 300.0) <= 1.0 and abs(by["m120.wav"]["drift_ppm"] + 120.0) <= 1.0
    assert by["p300.wav"]["drift_ok"] and by["m120.wav"]["drift_ok"] and by["late5.wav"]["drift_ok"] and not by["other.wav"]["drift_ok"]
    assert abs(by["p300.wav"]["lag_offset"] - 37.4) <= 0.05 and abs(by["m120.wav"]["lag_offset"] + 12.3) <= 0.05
    assert by["m120.wav"]["polarity"] == -1 and abs(by["late5.wav"]["drift_ppm"]) <= 1.0 and abs(by["late5.wav"]["lag_offset"] - 5.0) <= 0.05
    assert all(isinstance(r["drift_resid"], float) and np.isfinite(r["esr"]) for r in by.values())

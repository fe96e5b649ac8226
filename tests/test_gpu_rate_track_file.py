"""GPU: the rate contour at file level -- ``rate_track.fit_rate_track`` / ``synth_from_rate_track`` on the acceptance row of
tests/test_rate_track64.py, ``file_eval.score_pair(..., rate_track=...)`` on a synthetic recording whose LFO glides, and
``scripts/eval_pairs.py --rate_track`` as a child process.

1. The row tri 0.45 -> 0.7 Hz, noise 0.07 (the third row for which the fp64 helper passes every ratio; that module's docstring
   says why the 0.5 -> 0.6 Hz row at noise 0.10 cannot): ``fit_lfo`` on the whole row reports a resid at least 5 x
   ``fit_rate_track``'s mean slice resid, and ``synth_from_rate_track`` is within 2^-22 of the amplitude of the helper's stitched
   template.
2. tests/test_gpu_file_eval.py's 6 s recording with a triangle whose rate glides 0.9 -> 1.1 Hz and its stub extractor (the true
   LFO of every window).  ``score_pair(..., rate_track={...})`` returns the keys and the values of the call without it bit for bit,
   plus the new keys; ``fit/esr`` is finite and below the esr of a re-render from the single-rate ``synth_from_fit`` template of
   the same track -- the comparison the feature exists for.  Measured on the MI355X (profiles/r27/README.md): the track's own esr
   4.7e-4, ``fit/esr`` 0.107, the single-rate template's 0.331 (0.9993 Hz, resid 0.086); the contour runs 0.929 .. 1.070 Hz.
3. ``eval_pairs.py`` with and without ``--rate_track``: the keys both lines have are equal.
All FAIL WITHOUT THE FEATURE: neither the module nor the argument nor the flag exists."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import rate_track64 as r
from tests.test_gpu_file_eval import L, N, N_F, SR, spec_of
from tests.helpers.rate_track_cases import HOP, W, WINDOW, family_row, path_fit
from tests.helpers.rate_track_cases import N as ROW_N
from tests.helpers.rate_track_cases import SR as ROW_SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_acceptance_row_on_the_device(dev):
    from mod_extraction_amd import modulations as M, rate_track as R
    y, clean, f_true, starts = family_row("tri_0.45_0.7")
    ref = {"fit": path_fit("tri_0.45_0.7")}
    yd = torch.from_numpy(y).to(dev)
    single = M.fit_lfo(yd, ROW_SR, WINDOW)
    rt = R.fit_rate_track(yd, ROW_SR, W, HOP, WINDOW)
    got = R.synth_from_rate_track(rt).cpu().numpy().astype(np.float64)
    want = r.stitched(ref["fit"], ROW_SR, ROW_N)
    worst = float(np.abs(got - want).max()) / 0.7
    same = int((rt.grid_k[0].cpu().numpy() * 32 + rt.grid_j[0].cpu().numpy() == ref["fit"]["path"]).sum())
    print(f"device: single-rate resid {float(single.resid[0]):.4f}, mean slice resid {float(rt.resid.mean()):.4f}, rates "
          f"{[round(v, 3) for v in rt.rate_hz[0].tolist()]}; path equal to the helper's in {same} of {len(starts)} slices; stitched "
          f"template against the helper's: {worst:.3e} of the amplitude")
    assert rt.starts.tolist() == starts and int(rt.shape[0]) == ref["fit"]["shape"]
    assert float(single.resid[0]) >= 5.0 * float(rt.resid.mean())
    tol = 2.0 ** -22
    assert worst <= tol


def glide_truth(p):
    """The LFO at sample position p (fp64): a triangle between 0.1 and 0.9 whose rate glides 0.9 -> 1.1 Hz over the 6 s."""
    t = np.asarray(p, np.float64) / SR
    x = 0.9 * t + (0.2 / 12.0) * t * t + 0.15
    return 0.1 + 0.8 * (1.0 - 2.0 * np.abs(x - np.floor(x) - 0.5))


class GlideStub(torch.nn.Module):
    """tests/test_gpu_file_eval.Stub with ``glide_truth``: the true LFO of every window it is shown."""

    def __init__(self, wet_file):
        super().__init__()
        self.heads = wet_file.unfold(0, 16, 1)

    def forward(self, x):
        lfos = []
        for row in x[:, -1, :]:
            s = int((self.heads == row[:16]).all(1).nonzero()[0, 0])
            lfos.append(glide_truth(s + np.arange(N_F) * (N - 1) / (N_F - 1)).astype(np.float32))
        return torch.from_numpy(np.stack(lfos)).to(x.device).unsqueeze(1), torch.zeros(x.size(0), 4, 8, device=x.device)


def test_score_pair_with_a_rate_track(dev):
    from mod_extraction_amd import lightning, modulations as M
    from mod_extraction_amd.effect_losses import effect_loss_terms
    from mod_extraction_amd.file_eval import fit_track, render_file, score_pair
    from mod_extraction_amd.rate_track import RateTrack
    rng = np.random.default_rng(33)
    dry = torch.from_numpy((0.3 * rng.standard_normal(L)).astype(np.float32)).to(dev)
    fxp = {"feedback": 0.3, "min_delay_width": 0.5, "width": 0.8, "depth": 0.8, "mix": 0.7}
    mk = lambda **kw: lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=SR, effect="flanger",
                                                           audio_loss_dict={"esr": 1.0, "l1": 0.5}, **kw).to(dev)
    lfo_full = torch.from_numpy(glide_truth(np.arange(L)).astype(np.float32)).to(dev)
    wet = mk().render(dry.view(1, 1, L), lfo_full.view(1, L), fxp).reshape(L)
    stub = GlideStub(wet)
    # with the step's per-file match: the keys and values of the plain call, and the new keys
    step = mk(learned_fx=spec_of(fxp), match_gain="ls")
    plain = score_pair(step, stub, dry, wet, n_samples=N)
    both = score_pair(step, stub, dry, wet, n_samples=N, rate_track={"slice_s": 2.0, "hop_s": 1.0})
    assert list(both)[:len(plain)] == list(plain)
    for k, v in plain.items():
        assert torch.equal(v, both[k]) if isinstance(v, torch.Tensor) else v == both[k], k
    assert set(both) - set(plain) == {"rate_track", "rate_min_hz", "rate_max_hz", "rate_resid", "fit_wet_hat", "fit/esr", "fit/l1"}
    rt = both["rate_track"]
    n_t = plain["track"].numel()
    assert isinstance(rt, RateTrack) and (rt.slice_points, rt.n_points) == (345, n_t) and both["fit_wet_hat"].shape == (L,)
    assert 0.85 <= float(both["rate_min_hz"]) <= float(both["rate_max_hz"]) <= 1.15 and int(rt.shape[0]) == M.SHAPE_IDS["tri"]
    assert math.isfinite(float(both["fit/esr"])) and math.isfinite(float(both["fit/l1"]))
    # without a match: fit/esr against the re-render from the single-rate template of the same track
    bare = mk(learned_fx=spec_of(fxp))
    out = score_pair(bare, stub, dry, wet, n_samples=N, rate_track={"slice_points": 345, "hop_points": 172})
    point_rate = SR * (n_t - 1) / (L - 1)
    fit, _ = fit_track(out["track"], point_rate)
    one_rate = render_file(bare, dry, M.synth_from_fit(fit, n_t, point_rate)[0])
    rows = L // N
    esr_one = float(effect_loss_terms(one_rate[:rows * N].view(rows, 1, N), wet[:rows * N].view(rows, 1, N))["esr"])
    print(f"glide 0.9 -> 1.1 Hz: the track's own esr {float(out['esr']):.3e}, fit/esr {float(out['fit/esr']):.3e}, the single-rate "
          f"template ({float(fit.rate_hz[0]):.4f} Hz, resid {float(fit.resid[0]):.3f}) {esr_one:.3e}; contour "
          f"{[round(v, 3) for v in out['rate_track'].rate_hz[0].tolist()]} Hz, mean slice resid {float(out['rate_resid']):.2e}")
    assert math.isfinite(float(out["fit/esr"])) and float(out["fit/esr"]) < esr_one
    for bad in ({"hop_s": 1.0}, {"slice_s": 2.0, "slice_points": 345}, "2.0"):
        with pytest.raises(ValueError, match="score_pair"):
            score_pair(bare, stub, dry, wet, n_samples=N, rate_track=bad)


def test_eval_pairs_with_and_without_the_flag(dev, tmp_path):
    from scipy.io import wavfile
    from mod_extraction_amd import cli, lightning
    from tests.test_gpu_eval_pairs import CONFIG
    from tests.test_gpu_eval_pairs import N as CLIP
    from tests.test_gpu_eval_pairs import SR as RATE
    rng = np.random.default_rng(34)
    fxp = {"feedback": 0.3, "min_delay_width": 0.5, "width": 0.8, "depth": 0.8, "mix": 0.7}
    render = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), sr=RATE, effect="flanger")
    n = 40000
    for d in ("dry", "wet"):
        os.makedirs(tmp_path / d)
    dry = (0.3 * rng.standard_normal(n)).astype(np.float32)
    lfo = (0.5 + 0.4 * np.sin(2 * np.pi * 1.1 * np.arange(n) / RATE)).astype(np.float32)
    wet = render.render(torch.from_numpy(dry).to(dev).view(1, 1, n), torch.from_numpy(lfo).to(dev).view(1, n), fxp)
    wavfile.write(str(tmp_path / "dry" / "mid.wav"), RATE, dry)
    wavfile.write(str(tmp_path / "wet" / "mid.wav"), RATE, wet.reshape(n).cpu().numpy())
    cfg_path = tmp_path / "eval.yml"
    cfg_path.write_text(CONFIG.format(n=CLIP, sr=RATE, model=os.path.join(ROOT, "configs", "models", "spectral_2dcnn.yml")))
    torch.manual_seed(5)
    step = cli.instantiate(cli.apply_links(cli.load_config(str(cfg_path)))["model"])
    ckpt = tmp_path / "fresh.ckpt"
    torch.save({"state_dict": step.state_dict()}, str(ckpt))
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "eval_pairs.py"), "-c", str(cfg_path), "--ckpt", str(ckpt), "--dry_dir",
           str(tmp_path / "dry"), "--wet_dir", str(tmp_path / "wet"), "--batch_size", "4"]
    lines = []
    for extra in ([], ["--rate_track", "0.4:0.2"]):
        done = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=240)
        assert done.returncode == 0, done.stderr[-2000:]
        rows = [json.loads(l) for l in done.stdout.splitlines() if l.startswith("{")]
        assert len(rows) == 1
        lines.append(rows[0])
    off, on = lines
    print(on)
    assert all(on[k] == v for k, v in off.items()) and list(on)[:len(off)] == list(off)
    new = set(on) - set(off)
    assert new == {"rate_min_hz", "rate_max_hz", "rate_resid", "fit/esr", "fit/l1", "rate_shape", "rate_times_s", "rate_track_hz"}
    assert len(on["rate_times_s"]) == len(on["rate_track_hz"]) >= 2 and on["rate_min_hz"] == min(on["rate_track_hz"])
    assert all(math.isfinite(on[k]) for k in ("rate_min_hz", "rate_max_hz", "rate_resid", "fit/esr", "fit/l1"))

#!/usr/bin/env python3
"""Score a trained effect-rendered step on whole recordings: one JSON line per dry / wet file pair.

    python eval_pairs.py --config ../configs/train_lfo_pairs_flanger_fir.yml --ckpt run.ckpt --dry_dir DRY --wet_dir WET

The config's ``model`` must be a ``lightning.LFOExtractionThroughEffect`` (without ``fx_head``); its ``data`` section supplies
``n_samples``, ``sr`` and -- when ``align_max_lag_ms`` is there -- the alignment settings.  Files are paired as
``datasets.RandomAudioChunkDryWetDataset`` pairs them (same name in both directories, same rate, channels and length within
``end_buffer_n_samples``); with ``align_max_lag_ms`` its ``estimate_alignment`` table gives every pair's lag and polarity.
Recordings at another rate than the config's ``sr``: ``--resample_cache_dir DIR`` converts both directories on the device into
``DIR/dry`` and ``DIR/wet`` first (``resample.convert_tree``) and scores those; without it such files are dropped.
Per pair ``file_eval.score_pair`` runs on channel 0 of the whole file: the extractor's LFO track, the rate and shape fitted
to it, the re-render from the file's first sample, ONE gain or FIR for the file (and, with the step's
``match_shaper``, ONE curve: ``shaper``, its coefficients), and the step's audio losses.
``--rate_track SLICE_S[:HOP_S]`` also fits the track's rate contour (``rate_track.fit_rate_track`` on slices of SLICE_S seconds,
HOP_S apart, default half a slice) and adds ``rate_min_hz``, ``rate_max_hz``, ``rate_resid``, the per-slice ``rate_times_s`` and
``rate_track_hz``, and ``fit/<loss>``: the losses of a re-render from the clean LFO that contour describes.
``--drift``: for pairs whose two files ran on two clocks.  Per pair ``alignment.estimate_file_drift`` measures the line of lags
on the two whole files (they are on the device already; the config's ``align_max_lag_ms`` is its reach) and, where it is
trusted, ``score_pair`` warps the wet along it onto the dry's length instead of shifting it; the line gains ``drift_ppm``,
``lag_offset``, ``drift_resid`` and ``drift_ok``.  An untrusted pair is scored by its constant lag as without the flag.  Pairs
whose lengths differ by more than ``end_buffer_n_samples`` are still dropped by the pairing.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mod_extraction_amd import alignment, cli, datasets, file_eval, lightning, modulations, resample  # noqa: E402
from mod_extraction_amd import rate_track as rate_track_mod  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", "-c", required=True)
    ap.add_argument("--ckpt", required=True, help="Lightning .ckpt or a bare .pt state dict (cli.load_weights)")
    ap.add_argument("--dry_dir", required=True)
    ap.add_argument("--wet_dir", required=True)
    ap.add_argument("--hop", type=int, default=None, help="hop of the extractor's windows in samples (default n_samples // 2)")
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--resample_cache_dir", default=None,
                    help="bring both directories to the config's sr on the device, into DIR/dry and DIR/wet, and score those")
    ap.add_argument("--rate_track", default=None, metavar="SLICE_S[:HOP_S]",
                    help="also fit a rate contour on slices of SLICE_S seconds (HOP_S apart, default half a slice)")
    ap.add_argument("--drift", action="store_true",
                    help="estimate every pair's line of lags (two clocks) on the files and warp the wet along it")
    ap.add_argument("--drift_probe_points", type=int, default=8192)
    ap.add_argument("--drift_n_probes", type=int, default=16)
    a = ap.parse_args()
    rate_track = None
    if a.rate_track is not None:
        try:
            parts = [float(v) for v in a.rate_track.split(":")]
            assert len(parts) in (1, 2) and all(v > 0.0 for v in parts)
        except (ValueError, AssertionError):
            raise SystemExit(f"--rate_track takes SLICE_S or SLICE_S:HOP_S in seconds, got {a.rate_track!r}") from None
        rate_track = dict(zip(("slice_s", "hop_s"), parts))
    cfg = cli.apply_links(cli.load_config(a.config))
    dev = torch.device(a.device)
    step = cli.instantiate(cfg["model"]).to(dev)
    if not isinstance(step, lightning.LFOExtractionThroughEffect):
        raise SystemExit(f"the config's model is a {type(step).__name__}: eval_pairs scores an LFOExtractionThroughEffect")
    cli.load_weights(step, a.ckpt)
    step.eval()
    data = dict((cfg.get("data") or {}).get("init_args") or {})
    n_samples, sr = int(data.get("n_samples", 88200)), float(data.get("sr", step.sr))
    dry_dir, wet_dir = a.dry_dir, a.wet_dir
    if a.resample_cache_dir:
        if int(sr) != sr:
            raise SystemExit(f"--resample_cache_dir needs an integer sr, the config has {sr}")
        dry_dir, wet_dir = (os.path.join(a.resample_cache_dir, w) for w in ("dry", "wet"))
        resample.convert_tree(a.dry_dir, dry_dir, int(sr), device=dev)
        resample.convert_tree(a.wet_dir, wet_dir, int(sr), device=dev)
    ds = datasets.RandomAudioChunkDryWetDataset(
        dry_dir, wet_dir, n_samples, sr, check_dataset=False, end_buffer_n_samples=int(data.get("end_buffer_n_samples", 0)),
        align_max_lag_ms=data.get("align_max_lag_ms"), align_n_probes=int(data.get("align_n_probes", 8)),
        align_min_corr=float(data.get("align_min_corr", 0.5)))
    if a.drift and ds.align_max_lag is None:
        raise SystemExit("--drift needs the config's align_max_lag_ms: it is the reach of the estimate")
    table = ds.estimate_alignment(dev) if ds.align_max_lag is not None else {}
    for dry_path in ds.dry_paths:
        name = os.path.basename(dry_path)
        dry, wet = datasets.wav_load(dry_path)[0][0], datasets.wav_load(ds.name_to_wet_path[name])[0][0]
        n = min(dry.numel(), wet.numel())
        row = {"file": name, "samples": n}
        if n < n_samples:
            row["skipped"] = f"shorter than one window of {n_samples} samples"
            print(json.dumps(row), flush=True)
            continue
        al = table.get(name)
        lag, polarity = (al.lag, al.polarity) if al is not None else (0, 1)
        est = None
        if a.drift:
            dry_d, wet_d = dry.to(dev), wet.to(dev)
            est = alignment.estimate_file_drift(dry_d, wet_d, ds.align_max_lag, a.drift_probe_points, a.drift_n_probes,
                                                min_corr=ds.align_min_corr)
            row.update(drift_ppm=1e6 * est.drift, lag_offset=est.offset, drift_resid=est.resid, drift_ok=est.ok)
        if est is not None and est.ok:
            out = file_eval.score_pair(step, step.model, dry_d, wet_d, hop=a.hop, n_samples=n_samples, batch_size=a.batch_size,
                                       rate_track=rate_track, drift=est)
            lag, polarity = 0, est.polarity
        else:
            out = file_eval.score_pair(step, step.model, dry[:n].to(dev), wet[:n].to(dev), lag=lag, polarity=polarity, hop=a.hop,
                                       n_samples=n_samples, batch_size=a.batch_size, rate_track=rate_track)
        row.update(lag=lag, polarity=polarity, aligned=bool(al.ok) if al is not None else None,
                   n_windows=out["n_windows"], fit_points=out["fit_points"], track_points=int(out["track"].numel()),
                   rate_hz=float(out["rate_hz"]), shape=modulations.SHAPE_NAMES[int(out["shape"])], resid=float(out["resid"]))
        row.update({k: float(out[k]) for k in step.audio_loss_dict})
        if "fir" in out:
            row["fir"] = [float(v) for v in out["fir"]]
        if "gain" in out:
            row["gain"] = float(out["gain"])
        if "shaper" in out:
            row["shaper"] = [float(v) for v in out["shaper"]]
        if rate_track is not None:
            rt = out["rate_track"]
            row.update({k: float(out[k]) for k in ("rate_min_hz", "rate_max_hz", "rate_resid")})
            row.update({f"fit/{k}": float(out[f"fit/{k}"]) for k in step.audio_loss_dict})
            row["rate_shape"] = modulations.SHAPE_NAMES[int(rt.shape[0])]
            row["rate_times_s"] = [float(v) for v in rate_track_mod.rate_at(rt)[0]]
            row["rate_track_hz"] = [float(v) for v in rt.rate_hz[0]]
        print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

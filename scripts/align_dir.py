#!/usr/bin/env python3
"""Put the wet files of recorded dry / wet pairs on their dry files' time base, on the device: one JSON line per pair.

    python align_dir.py --dry_dir DRY --wet_dir WET --out_dir WET_ON_DRY_CLOCK --sr 44100 --max_lag_ms 50

``alignment.warp_tree`` (K26): for every ``*ext`` file under ``--dry_dir`` and the file at the same relative path under
``--wet_dir``, the line of lags over the file is estimated (``estimate_file_drift``: short probes, K19's correlation, a
Theil-Sen line) and the wet appears under that path in ``--out_dir`` as a float32 RIFF with the dry's frame count and the
polarity applied -- warped along the line, shifted by whole samples when the pair shows no drift (bit-exact samples), or
copied byte for byte when the estimate is not trusted.  A pair converted by an earlier run (same sources, same settings) is
left alone.  The data modules' ``align_drift_cache_dir`` key does the same at ``setup``.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mod_extraction_amd import alignment  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dry_dir", required=True)
    ap.add_argument("--wet_dir", required=True)
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--sr", type=int, required=True)
    ap.add_argument("--max_lag_ms", type=float, required=True, help="the reach of the estimate: |offset| + |drift| * length")
    ap.add_argument("--ext", default="wav")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--probe_points", type=int, default=8192)
    ap.add_argument("--n_probes", type=int, default=16)
    ap.add_argument("--min_corr", type=float, default=0.5)
    ap.add_argument("--max_resid", type=float, default=0.5)
    ap.add_argument("--min_drift_samples", type=float, default=0.25)
    ap.add_argument("--zeros", type=int, default=48)
    ap.add_argument("--rolloff", type=float, default=0.95)
    ap.add_argument("--beta", type=float, default=16.0)
    a = ap.parse_args()
    done = alignment.warp_tree(a.dry_dir, a.wet_dir, a.out_dir, a.sr, int(round(a.max_lag_ms * 1e-3 * a.sr)), ext=a.ext,
                               device=torch.device(a.device), min_drift_samples=a.min_drift_samples, probe_points=a.probe_points,
                               n_probes=a.n_probes, min_corr=a.min_corr, max_resid=a.max_resid, zeros=a.zeros, rolloff=a.rolloff,
                               beta=a.beta)
    for rel, p in done.items():
        print(json.dumps({"file": rel, "offset": p.offset, "drift_ppm": 1e6 * p.drift, "polarity": p.polarity, "corr": p.corr,
                          "resid": p.resid, "n_probes": p.n_probes, "ok": p.ok}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

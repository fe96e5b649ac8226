#!/usr/bin/env python3
"""Bring a directory of wav files to one sample rate on the device: one JSON line per file.

    python resample_dir.py --in_dir RAW_48K --out_dir AT_44100 --sr 44100

``resample.convert_tree`` (K24): every ``*ext`` file under ``--in_dir`` appears under the same relative path in ``--out_dir`` as
a float32 RIFF at ``--sr`` -- converted by the band-limited rational resampler, or copied byte for byte when it is at that
rate already.  A file converted by an earlier run (same source size and mtime, same rate and filter) is left alone.  The
file-backed datasets drop files that are not at their ``sr``; the data modules' ``resample_cache_dir`` key does the same
conversion at ``setup``.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mod_extraction_amd import resample  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--in_dir", required=True)
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--sr", type=int, required=True)
    ap.add_argument("--ext", default="wav")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--zeros", type=int, default=48)
    ap.add_argument("--rolloff", type=float, default=0.95)
    ap.add_argument("--beta", type=float, default=16.0)
    a = ap.parse_args()
    done = resample.convert_tree(a.in_dir, a.out_dir, a.sr, ext=a.ext, device=torch.device(a.device), zeros=a.zeros,
                                 rolloff=a.rolloff, beta=a.beta)
    for src, (sr_in, frames_in, frames_out) in done.items():
        print(json.dumps({"file": os.path.relpath(src, a.in_dir), "sr_in": sr_in, "sr_out": a.sr, "frames_in": frames_in,
                          "frames_out": frames_out}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

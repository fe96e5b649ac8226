"""Timing of the tremolo kernels (mx_tremolo_fwd, mx_tremolo_bwd) with HIP events, fixed seed, at 256 x 88 200 samples
with the 882-point LFO of the data path.  Prints:

  (a) mx_tremolo_fwd: time, achieved bytes/s at 8 B/sample (x in, y out; the LFO row is 1 % of that) and its fraction of
      the HBM peak bench.py's roofline uses
  (b) mx_tremolo_bwd with dx, dmod and dmix: time, achieved bytes/s at 12 B/sample (dy, x in, dx out), the same fraction
  (c) mx_tremolo_bwd asked for dmod alone (what the audio-loss step runs): time, bytes/s at 8 B/sample (dy, x in)
  (d) the torch route these replace: util.linear_interpolate_last_dim + the elementwise expression of fx.py:22 for the
      forward, torch autograd through both for the backward, with the ratios to (a) and (b)

No ratio is gated anywhere; this tool is how the numbers in profiles/ are produced.

    python tools/tremolo_time.py [--reps 20]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_PEAK_GBPS = 8000.0                      # bench.py's roofline peak (MI355X)


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def rate(label, ms, bytes_per_sample, samples):
    gbps = bytes_per_sample * samples / (ms * 1e-3) / 1e9
    print(f"{label}: {ms:.4f} ms, {gbps:.0f} GB/s at {bytes_per_sample} B/sample = {gbps / HBM_PEAK_GBPS:.3f} of the "
          f"{HBM_PEAK_GBPS:.0f} GB/s HBM peak")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from mod_extraction_amd import fx, util
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, N, n_mod = 256, 88200, 882
    x = torch.rand(B, N, device=dev) * 2 - 1
    mod = torch.rand(B, n_mod, device=dev)
    dy = torch.randn(B, N, device=dev)
    mix = torch.rand(B, device=dev)
    c = fx.derive_tremolo_constants(B, dev, mix)
    y = torch.empty_like(x)

    t_fwd = timed(lambda: fx.tremolo_forward(x, mod, c, out=y), args.reps)
    t_bwd = timed(lambda: fx.tremolo_backward(dy, x, mod, c), args.reps)
    t_dmod = timed(lambda: fx.tremolo_backward(dy, x, mod, c, need_dx=False, need_dmix=False), args.reps)
    rate("(a) mx_tremolo_fwd", t_fwd, 8, B * N)
    rate("(b) mx_tremolo_bwd (dx, dmod, dmix)", t_bwd, 12, B * N)
    rate("(c) mx_tremolo_bwd (dmod alone)", t_dmod, 8, B * N)

    def torch_fwd(x_, mod_, mix_):
        m = util.linear_interpolate_last_dim(mod_, N, align_corners=True)
        return ((1.0 - mix_[:, None]) * x_) + (mix_[:, None] * m * x_)

    assert torch.equal(torch_fwd(x, mod, mix), y)
    t_tfwd = timed(lambda: torch_fwd(x, mod, mix), args.reps)

    def interp(m_):                          # differentiable stand-in for the resampling (torch's own, same rule)
        return torch.nn.functional.interpolate(m_[:, None], N, mode="linear", align_corners=True)[:, 0]

    xg, mg, wg = x.clone().requires_grad_(True), mod.clone().requires_grad_(True), mix.clone().requires_grad_(True)

    def torch_bwd():
        xg.grad = mg.grad = wg.grad = None
        out = ((1.0 - wg[:, None]) * xg) + (wg[:, None] * interp(mg) * xg)
        out.backward(dy)

    t_tbwd = timed(torch_bwd, args.reps)
    print(f"(d) torch route: forward (mx_interp_linear + 5 elementwise ops) {t_tfwd:.4f} ms = {t_tfwd / t_fwd:.2f}x (a); "
          f"forward + autograd backward (F.interpolate) {t_tbwd:.4f} ms = {t_tbwd / (t_fwd + t_bwd):.2f}x (a) + (b)")


if __name__ == "__main__":
    main()

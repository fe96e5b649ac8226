"""GPU: the log-mel front end (mx_logmel_fwd: melspec_kernel for n_fft 1024, melspec_wf_kernel<512> / <2048>) against
an fp64 evaluation written from the definitions (tests/helpers/fp64_refs.py: reflect pad, periodic Hann, numpy rfft,
|X|^2, @ fb, masks, clip, log) that shares no code with the product or the oracle.  The reference applies the module's
OWN filter bank and window promoted to fp64: applying the tables is the kernel's job; the tables themselves are checked
against the closed-form HTK triangles and the periodic Hann window in tests/test_fp64_refs.py.

Gates (per call):
  * linear power, per (clip, channel) plane:  max|exp(got) - clip(M64, eps)| / max|M64| <= 1e-5
  * live cells (M64 above the floor):  |got - log M64| <= max(2e-6, 3 x the error of the same pipeline run in plain fp32
    (scipy.fft on float32), the yardstick of what fp32 can reach on these inputs) -- or 3 x the cell's fp32 conditioning
    where that is larger (see check(): a band of weak bins beside a loud frame; a second fp32 FFT, torch.stft, misses the
    yardstick gate there by 4x on the 11-frame clips, so the plane-wide yardstick alone cannot bound such a cell)
  * cells below the floor come out exactly the clip value log(eps) (one value, bit-identical everywhere), except where the
    fp64 value lies within 1e-5 (relative) or within 3 x the cell's fp32 conditioning of the floor
  * padding columns >= n_frames are exactly 0
"""
import math

import numpy as np
import pytest
import torch

from tests.helpers import fp64_refs as R

pytestmark = pytest.mark.gpu

EPS = 1e-7
N_MELS = {512: 64, 1024: 256, 2048: 256}
HOPS = {512: (1, 100, 256, 512, 1024), 1024: (1, 100, 256, 1024, 2048), 2048: (1, 100, 256, 2048, 4096)}


def module(dev, n_fft, hop, sr=44100, n_mels=None):
    from mod_extraction_amd import models as am
    return am.MelSpectrogramHIP(sr, n_fft, hop, n_mels or N_MELS[n_fft]).to(dev)


def signals(N, n_fft, seed=0):
    """(S, N) float32: one row per signal kind."""
    g = np.random.default_rng(seed)
    n = np.arange(N, dtype=np.float64)
    k0 = n_fft // 8 + 3
    rows = [
        g.uniform(-0.5, 0.5, N),                                          # white noise
        0.8 * np.sin(2 * math.pi * k0 / n_fft * n + 0.3),                 # sine centred on bin k0
        0.8 * np.sin(2 * math.pi * (k0 + 0.5) / n_fft * n + 1.1),         # sine half-way between two bins
        0.5 + 0.05 * g.uniform(-1, 1, N),                                 # DC offset: bin 0
        0.6 * np.where(np.arange(N) % 2 == 0, 1.0, -1.0),                 # +-a alternating: the Nyquist bin n_fft/2
        np.zeros(N),                                                      # impulses at the two clip ends (reflect pad)
        np.zeros(N),                                                      # silence
        np.where(np.sin(2 * math.pi * n / 97.0 + 0.1) >= 0, 1.0, -1.0),   # full-scale square wave
    ]
    rows[5][0], rows[5][-1] = 1.0, -0.7
    return np.stack(rows).astype(np.float32)


SILENCE = 6


def n_frames_of(N, hop):
    return N // hop + 1


def lengths(n_fft, hop):
    """Clip lengths: the shortest the ABI accepts, n_fft, n_fft + 1, and three whose frame counts are 0, 1, 15 mod 16
    (MEL_FR = 16 frames per workgroup)."""
    out = [n_fft // 2 + 1, n_fft, n_fft + 1]
    for r in (0, 1, 15):
        q = 1
        while hop * (16 * q + r - 1) <= n_fft // 2 + 1:
            q += 1
        out.append(hop * (16 * q + r - 1) + hop // 2)
    return out


def check(got, x, mod, n_fft, hop, n_frames, eps=EPS, masks=(0, 0, 0, 0), fb=None, tag=""):
    """got (P, n_mels, pitch) float32 from the kernel, x (P, N) float32; the reference applies the module's own window
    and filter bank (fb: the bank the kernel was given, default the module's) promoted to fp64.  (The window table is
    torch.hann_window, torchaudio's, whose fp32 edge taps are up to 5.5e-4 off in relative terms -- 2e-7 absolute,
    tests/test_fp64_refs.py -- which an impulse under an edge tap would show as a kernel error.)"""
    got = np.asarray(got)
    assert np.all(got[..., n_frames:] == 0), tag
    got = got[..., :n_frames].astype(np.float64)
    fb = np.asarray(mod.mel_scale.fb.cpu().numpy() if fb is None else fb, dtype=np.float64)
    win = mod.spectrogram.window.cpu().numpy()
    L64, M64 = R.logmel64(x.astype(np.float64), n_fft, hop, fb, eps, masks, n_frames, window=win)
    L32, _ = R.logmel64(x, n_fft, hop, fb.astype(np.float32), eps, masks, n_frames, dtype=np.float32, window=win)
    f0, f1, t0, t1 = masks
    live_mask = np.ones(M64.shape[-2:], dtype=bool)
    live_mask[f0:f1, :] = False
    live_mask[:, t0:t1] = False
    Mm = np.where(live_mask, M64, 0.0)
    eps32 = float(np.float32(eps))
    floor = float(np.float32(math.log(eps32)))
    # fp32 conditioning of each cell: a transform in fp32 leaves an absolute error of about u * log2(n_fft) * ||x_w||_2 in
    # every bin (||x_w||_2 = sqrt(sum of the windowed frame's squares), u = 2^-24); a bin of amplitude |X_k| then carries
    # 2 |X_k| of it in its power, and a band sums those through fb: cond = sum_k fb_k 2 |X_k| delta / M is the relative
    # error that fp32 input rounding alone puts on a cell (bands of weak single bins next to a loud frame: 1e-5 and more).
    P64 = R.power_spectrum(x.astype(np.float64), n_fft, hop, n_frames, window=win)      # (P, F, K)
    fr = R.frames_reflect(x.astype(np.float64), n_fft, hop, n_frames) * win.astype(np.float64)
    delta = 2.0 ** -24 * math.log2(n_fft) * np.sqrt((fr * fr).sum(-1))                  # (P, F)
    cond_abs = np.swapaxes((2.0 * np.sqrt(P64) * delta[..., None]) @ fb, -1, -2)          # (P, n_mels, F)
    res = {}
    for p in range(got.shape[0]):
        g, m, mm, l32 = got[p], M64[p], Mm[p], L32[p].astype(np.float64)
        scale = float(np.abs(m).max())
        if scale > 0:
            lin = float(np.abs(np.exp(g) - np.maximum(mm, eps32)).max()) / scale
            assert lin <= 1e-5, (tag, p, lin)
            res["lin"] = max(res.get("lin", 0.0), lin)
        live = mm > eps32 * (1 + 1e-5)
        if live.any():
            lm = np.log(mm[live])
            err = np.abs(g[live] - lm)
            e32 = float(np.abs(l32[live] - lm).max())
            cond = cond_abs[p][live] / mm[live]
            gate = np.maximum(max(2e-6, 3.0 * e32), 3.0 * cond)
            worst = int(np.argmax(err / gate))
            e_w, c_w = float(err[worst]), float(cond[worst])
            assert e_w <= max(2e-6, 3.0 * e32, 3.0 * c_w), (tag, p, e_w, e32, c_w)
            res["live"] = max(res.get("live", 0.0), float(err.max()))
            res["live_over_gate"] = max(res.get("live_over_gate", 0.0), float(err[worst] / gate[worst]))
        # below the floor: exempt where the fp64 value lies within 1e-5 of the floor or within the cell's fp32
        # conditioning of it (3 cond_abs, as above: a near-floor band that a bin's rounding can lift over eps)
        below = (mm < eps32 * (1 - 1e-5)) & (eps32 - mm > 3.0 * cond_abs[p])
        if below.any():
            vals = np.unique(g[below])
            assert vals.size == 1, (tag, p, vals[:8])
            assert abs(float(vals[0]) - floor) <= abs(float(np.spacing(np.float32(floor)))), (tag, p, float(vals[0]), floor)
    return res


def run(mod, x, n_frames, eps=EPS, masks=(0, 0, 0, 0), pitch=None):
    """x (P, N) float32 numpy -> (P, n_mels, pitch) numpy from MelSpectrogramHIP.log_mel (a pitch that is not a
    multiple of 16 frames: the padding columns end inside a workgroup's tile)."""
    pitch = pitch or n_frames + 7
    xt = torch.from_numpy(x).to(mod.twiddle.device)
    out = mod.log_mel(xt.unsqueeze(1) if x.ndim == 2 else xt, n_frames, eps, masks, pitch=pitch)
    return (out[:, 0] if x.ndim == 2 else out).cpu().numpy()


@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
@pytest.mark.parametrize("hop_i", range(5))
def test_logmel_signals_and_geometry_vs_fp64(dev, n_fft, hop_i):
    hop = HOPS[n_fft][hop_i]
    mod = module(dev, n_fft, hop)
    worst = {}
    for N in lengths(n_fft, hop):
        nf = n_frames_of(N, hop)
        x = signals(N, n_fft, seed=N)
        got = run(mod, x, nf)
        assert np.all(got[SILENCE, :, :nf] == got[SILENCE, 0, 0]), "silence is not one constant"
        for k, v in check(got, x, mod, n_fft, hop, nf, tag=(n_fft, hop, N)).items():
            worst[k] = max(worst.get(k, 0.0), v)
    assert worst["lin"] <= 1e-5
    assert worst["live_over_gate"] <= 1.0


def test_logmel_shipped_shape_vs_fp64(dev):
    """The headline front end: 88 200 samples x 2 channels, n_fft 1024, hop 256, 256 bands, 345 frames, pitch 352."""
    mod = module(dev, 1024, 256)
    x = signals(88200, 1024, seed=7)
    x2 = np.stack([x, 0.7 * x[:, ::-1]], axis=1)                            # (S, 2, N)
    nf = 345
    out = run(mod, np.ascontiguousarray(x2), nf, pitch=352)
    assert out.shape == (x.shape[0], 2, 256, 352)
    res = check(out.reshape(-1, 256, 352), x2.reshape(-1, 88200), mod, 1024, 256, nf)
    assert res["lin"] <= 1e-5
    assert res["live_over_gate"] <= 1.0


@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
def test_logmel_mask_ranges_vs_fp64(dev, n_fft):
    hop = 256
    mod = module(dev, n_fft, hop)
    n_mels = N_MELS[n_fft]
    N = 9000
    nf = n_frames_of(N, hop)
    x = signals(N, n_fft, seed=3)
    for masks in [(5, 5, 0, 0), (0, n_mels, 0, 0), (n_mels - 1, n_mels, nf - 1, nf), (0, 0, 15, 17), (3, 9, 15, 17)]:
        got = run(mod, x, nf, masks=masks)
        check(got, x, mod, n_fft, hop, nf, masks=masks, tag=(n_fft, masks))
        f0, f1, t0, t1 = masks
        assert np.all(got[:, f0:f1, :nf] == got[SILENCE, 0, 0])                 # masked cells sit on the clip value
        assert np.all(got[:, :, t0:t1] == got[SILENCE, 0, 0])


def _coef_cap(n_fft, n_mels):
    return 2 * (n_fft // 2 + 1) + 2 * n_mels                                   # melspec.hip: the packed-LDS budget


def _support(fb):
    """Total width of the bands' non-zero row ranges [lo, hi): what the kernel packs into LDS."""
    nz = fb != 0
    tot = 0
    for m in range(fb.shape[1]):
        rows = np.nonzero(nz[:, m])[0]
        if rows.size:
            tot += rows[-1] + 1 - rows[0]
    return tot


def _load_fb(mod, fb):
    sd = mod.state_dict()
    sd["mel_scale.fb"] = torch.from_numpy(np.ascontiguousarray(fb, dtype=np.float32))
    mod.load_state_dict(sd)


@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
def test_logmel_checkpoint_banks_vs_fp64(dev, n_fft):
    """Filter banks a checkpoint may carry in ``spectrogram.mel_scale.fb``: a dense random bank (more coefficients than
    the packed-LDS budget: the kernels read fb from global memory), a sparse one (zeros inside bands, whole empty
    columns), loaded into a module that has already run, so that the output must follow the new bank (bands() cache)."""
    hop = 256
    mod = module(dev, n_fft, hop)
    n_bins, n_mels = n_fft // 2 + 1, N_MELS[n_fft]
    N = 7000
    nf = n_frames_of(N, hop)
    x = signals(N, n_fft, seed=11)
    htk = mod.mel_scale.fb.cpu().numpy().copy()
    assert _support(htk) <= _coef_cap(n_fft, n_mels)                       # the shipped bank: packed path
    check(run(mod, x, nf), x, mod, n_fft, hop, nf, fb=htk, tag="htk")

    g = np.random.default_rng(n_fft)
    dense = (g.uniform(0, 1, (n_bins, n_mels)) / n_bins * 4).astype(np.float32)
    assert _support(dense) > _coef_cap(n_fft, n_mels)                      # forces the global-fb branch
    _load_fb(mod, dense)
    got = run(mod, x, nf)
    check(got, x, mod, n_fft, hop, nf, fb=dense, tag="dense")

    # (the top bins and bands stay whole: the +-a signal's power sits in the two top bins alone, and with their bands
    # emptied the plane's max|M64| would be leakage at the fp64 noise level -- no scale for the linear gate)
    sparse = htk.copy()
    holes = g.uniform(0, 1, sparse.shape) < 0.3
    holes[-16:] = False
    sparse[holes] = 0.0                                                    # holes inside bands
    empty = 2 + g.choice(n_mels - 10, size=max(2, n_mels // 8), replace=False)
    sparse[:, empty] = 0.0                                                 # whole empty columns
    sparse[:, 1] = 0.0
    sparse[n_bins // 3, 1] = 0.5                                           # a one-bin band
    _load_fb(mod, sparse)
    got = run(mod, x, nf)
    check(got, x, mod, n_fft, hop, nf, fb=sparse, tag="sparse")
    assert np.all(got[:, empty, :nf] == got[SILENCE, 0, 0])

    _load_fb(mod, dense)                                                   # and back: the cached band limits follow
    check(run(mod, x, nf), x, mod, n_fft, hop, nf, fb=dense, tag="dense again")


@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
def test_logmel_rejects_bad_hop_and_frame_count_before_any_launch(dev, n_fft):
    """mx_logmel_fwd: hop <= 0, n_frames < 0 and n_frames > N/hop + 1 (frames whose reflect index would leave the
    clip) are MX_ERR_ARG, returned before any launch; n_frames = N/hop + 1 is accepted."""
    from mod_extraction_amd import _hip
    n_mels, N, hop = N_MELS[n_fft], 5000, 300
    mod = module(dev, n_fft, hop)
    lo, hi = mod.bands()
    x = torch.zeros(2, N, device=dev)
    out = torch.zeros(2, n_mels, 64, device=dev)

    def call(h, nf):
        return _hip.load().mx_logmel_fwd(_hip.ptr(x), 2, N, _hip.ptr(mod.spectrogram.window), _hip.ptr(mod.twiddle),
                                         _hip.ptr(mod.mel_scale.fb), _hip.ptr(lo), _hip.ptr(hi), n_fft, h, n_mels, nf,
                                         64, EPS, 0, 0, 0, 0, _hip.ptr(out), _hip.stream())
    assert call(0, 17) == -1                                               # MX_ERR_ARG
    assert call(-256, 17) == -1
    assert call(hop, N // hop + 2) == -1
    assert call(hop, 60) == -1
    assert call(hop, -1) == -1
    assert call(hop, N // hop + 1) == 0
    torch.cuda.synchronize()
    assert float(out[:, :, N // hop + 1:].abs().max()) == 0.0

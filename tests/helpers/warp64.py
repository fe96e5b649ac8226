"""numpy fp64 restatement of K26 (mod_extraction_amd/csrc/warp_abi.h has the definition): the warp along a straight line of
positions, ``alignment.fit_lag_line``'s rule, the probe estimate on tests/helpers/pair_align64.py, and the two recorded pairs
the CPU and GPU tests share.  Written from the header's text with numpy only.

The pairs.  3 s at 44.1 kHz: pink noise band-limited to 16 kHz, a feedback-free flanger with a 1 .. 10 ms tap rendered over
the whole file by tests/helpers/flanger_adjoint64.forward, and the wet then "recorded on another clock" by this module's own
warp along the inverse line: wet_rec[j] = pol * wet((j - offset) / (1 + drift)).  ``esr`` leaves ``TRIM`` samples out at
both ends of a file: there the recording does not hold the samples the line asks for (a wet that starts 12 samples early
has lost them), which says nothing about the estimate or the warp."""
import functools
import math
from typing import NamedTuple

import numpy as np

from tests.helpers import flanger_adjoint64 as fa
from tests.helpers import pair_align64
from tests.helpers import resample64

OUT_TILE = 1024
MAX_DRIFT = 1e-3
SR = 44100
L = 3 * SR
PROBE, N_PROBES, MAX_LAG = 8192, 12, 128
TRIM = 256                                                       # >= MAX_LAG + half
M_DELAY = 44 + 441                                               # the delay line of a 1 ms + 10 ms flanger at 44.1 kHz
# name -> (drift, offset, polarity, frames of the wet beyond the dry's)
PAIRS = {"p300": (300e-6, 37.4, 1, 40), "m120": (-120e-6, -12.3, -1, 0)}


def plan(zeros: int = 48, rolloff: float = 0.95):
    """(half, T)"""
    half = int(math.ceil(zeros / rolloff))
    return half, 2 * half + 1


def i0(x: np.ndarray) -> np.ndarray:
    """K24's series on an array: every element takes the terms its own stopping rule asks for, so each value is the scalar
    ``resample64.i0``'s to the bit."""
    x = np.asarray(x, dtype=np.float64)
    q = (0.25 * x * x).ravel()
    term, total = np.ones_like(q), np.ones_like(q)
    live = np.arange(q.size)
    for j in range(1, 1000):
        t = term[live] * q[live] / (float(j) * float(j))
        s = total[live] + t
        term[live], total[live] = t, s
        live = live[~(t < s * 2.0 ** -60)]
        if live.size == 0:
            break
    return total.reshape(x.shape)


def prototype(tau, half: int, c: float = 0.95, beta: float = 16.0) -> np.ndarray:
    """h(tau), tau in input samples (fp64 array)."""
    tau = np.asarray(tau, dtype=np.float64)
    inside = np.abs(tau) <= half
    r = np.where(inside, tau / half, 0.0)
    w = i0(beta * np.sqrt(np.maximum(0.0, 1.0 - r * r))) / float(i0(np.float64(beta)))
    return np.where(inside, c * np.sinc(c * tau) * w, 0.0)


def positions(n_out: int, offset: float, drift: float, m0: int = 0):
    """(i0, f) of the outputs m0 .. m0 + n_out - 1: pos = m + (m drift + offset), three roundings."""
    m = np.arange(m0, m0 + n_out, dtype=np.float64)
    pos = m + (m * np.float64(drift) + np.float64(offset))
    fl = np.floor(pos)
    return fl.astype(np.int64), pos - fl


def taps(f, half: int, c: float = 0.95, beta: float = 16.0) -> np.ndarray:
    """(n, T) fp64: h(f + (half - k))."""
    j = (half - np.arange(2 * half + 1)).astype(np.float64)
    return prototype(np.asarray(f, dtype=np.float64)[:, None] + j[None, :], half, c, beta)


def rows(x, offset, drift, n_out=None, sign=None, zeros: int = 48, rolloff: float = 0.95, beta: float = 16.0,
         with_bound: bool = False, chunk: int = 8192):
    """(B, n_out) fp64 from x (B, n_in) or (n_in,): y[m] = s sum_k h(f + half - k) x[i0 - half + k] in ascending k, x zero
    outside the row.  ``offset``, ``drift``, ``sign``: scalars or (B,).  ``with_bound`` adds (sum |h x|, sum |x|) over the taps'
    samples."""
    x = np.asarray(x, dtype=np.float64)
    one = x.ndim == 1
    x = np.atleast_2d(x)
    B, n_in = x.shape
    n_out = n_in if n_out is None else n_out
    half, T = plan(zeros, rolloff)
    offset, drift = np.broadcast_to(np.asarray(offset, np.float64), (B,)), np.broadcast_to(np.asarray(drift, np.float64), (B,))
    sign = np.ones(B) if sign is None else np.where(np.broadcast_to(np.asarray(sign, np.float64), (B,)) < 0, -1.0, 1.0)
    y, a, ax = (np.zeros((B, n_out)) for _ in range(3))
    k = np.arange(T)
    for b in range(B):
        for m0 in range(0, n_out, chunk):
            n = min(chunk, n_out - m0)
            i0_, f = positions(n, offset[b], drift[b], m0)
            h = taps(f, half, rolloff, beta)
            idx = i0_[:, None] - half + k[None, :]
            inside = (idx >= 0) & (idx < n_in)
            xs = np.where(inside, x[b][np.clip(idx, 0, n_in - 1)], 0.0)
            acc, s1, s2 = np.zeros(n), np.zeros(n), np.zeros(n)
            for kk in range(T):                                  # ascending k, as the kernel sums
                t = h[:, kk] * xs[:, kk]
                acc += t
                s1 += np.abs(t)
                s2 += np.abs(xs[:, kk])
            y[b, m0:m0 + n], a[b, m0:m0 + n], ax[b, m0:m0 + n] = sign[b] * acc, s1, s2
    if one:
        y, a, ax = y[0], a[0], ax[0]
    return (y, a, ax) if with_bound else y


def gate(y64, a, ax, T: int):
    """The bound on |y - y64| of the header: one fp32 rounding, two fp64 sums of T terms, 2^-40 a tap."""
    return 2.0 ** -24 * np.abs(y64) + T * 2.0 ** -53 * a + 2.0 ** -40 * ax


# ---- the line ------------------------------------------------------------------------------------------------------------
class Line(NamedTuple):
    offset: float
    drift: float
    polarity: int
    corr: float
    resid: float
    n_probes: int
    ok: bool


def fit_lag_line(centres, lags, corrs, min_corr=0.5, max_resid=0.5, min_probes=3) -> Line:
    """Theil-Sen as ``alignment.fit_lag_line`` states it, written with Python loops."""
    probes = [(float(c), float(l), float(r)) for c, l, r in zip(centres, lags, corrs)]
    med = float(np.median([abs(r) for _, _, r in probes])) if probes else 0.0
    kept = [p for p in probes if p[2] != 0.0 and abs(p[2]) >= min_corr]
    slopes = [(b[1] - a[1]) / (b[0] - a[0]) for i, a in enumerate(kept) for b in kept[i + 1:] if a[0] != b[0]]
    if len(kept) < min_probes or not slopes:
        return Line(0.0, 0.0, 1, med, 0.0, len(kept), False)
    drift = float(np.median(slopes))
    offset = float(np.median([l - drift * c for c, l, _ in kept]))
    resid = max(abs(l - (offset + drift * c)) for c, l, _ in kept)
    if med < min_corr or resid > max_resid:
        return Line(0.0, 0.0, 1, med, resid, len(kept), False)
    return Line(offset, drift, -1 if sum(r for _, _, r in kept) < 0.0 else 1, med, resid, len(kept), True)


def probes(dry, wet, max_lag: int = MAX_LAG, probe_points: int = PROBE, n_probes: int = N_PROBES):
    """(centres, lags, fracs, corrs) of ``alignment.estimate_file_drift``'s probes, each by pair_align64.estimate64."""
    span = min(len(dry), len(wet)) - probe_points
    hop = span // (n_probes - 1)
    out = []
    for k in range(n_probes):
        s = k * hop
        e = pair_align64.estimate64(dry[s:s + probe_points], wet[s:s + probe_points], max_lag)
        out.append((s + (probe_points - 1) / 2.0, e["lag"], e["frac"], e["corr"]))
    return tuple(np.array(v) for v in zip(*out))


def estimate(dry, wet, max_lag: int = MAX_LAG, probe_points: int = PROBE, n_probes: int = N_PROBES, **kw) -> Line:
    c, l, f, r = probes(dry, wet, max_lag, probe_points, n_probes)
    return fit_lag_line(c, l + f, r, **kw)


# ---- the pairs -----------------------------------------------------------------------------------------------------------
def lfo(n: int = L) -> np.ndarray:
    """A 0.7 Hz sine between 0.05 and 0.95, fp32."""
    return (0.5 + 0.45 * np.sin(2.0 * np.pi * 0.7 * np.arange(n) / SR + 0.3)).astype(np.float32)


def flanger_consts():
    """fx.derive_clip_constants for min_delay_width 1, width 0.9, feedback 0, depth 1, mix 0.5 at 44 + 441 samples."""
    f = lambda v: np.array([v], dtype=np.float32)
    return {"lfo_scale": f(0.9 * 441), "min_delay": f(1.0 * 44), "feedback": f(0.0), "depth": f(1.0), "mix": f(0.5),
            "one_minus_mix": f(1.0 - 0.5)}


FX_PARAMS = {"feedback": 0.0, "min_delay_width": 1.0, "width": 0.9, "depth": 1.0, "mix": 0.5}


@functools.lru_cache(maxsize=None)
def source():
    """(dry fp32 (L,), wet fp64 (L,)): the dry file and its undrifted render."""
    rng = np.random.default_rng(2601)
    spec = np.fft.rfft(rng.standard_normal(L))
    freq = np.fft.rfftfreq(L, 1.0 / SR)
    spec[1:] /= np.sqrt(freq[1:])
    spec[0] = 0.0
    spec[freq > 16000.0] = 0.0
    x = np.fft.irfft(spec, L)
    dry = (0.1 * x / np.sqrt(np.mean(x * x))).astype(np.float32)
    wet = fa.forward(dry[None, :], lfo()[None, :], flanger_consts(), M_DELAY)["y"][0]
    assert float(np.abs(wet).max()) < 1.0                        # the clip of the effect's output stays out of it
    dry.setflags(write=False)
    wet.setflags(write=False)
    return dry, wet


@functools.lru_cache(maxsize=None)
def recorded(name: str) -> np.ndarray:
    """The wet file of a pair, fp32: the render read along the inverse of the pair's line, times its polarity."""
    drift, offset, pol, extra = PAIRS[name]
    _, wet = source()
    inv = 1.0 / (1.0 + drift)
    rec = (pol * rows(wet, -offset * inv, inv - 1.0, n_out=L + extra)).astype(np.float32)
    rec.setflags(write=False)
    return rec


def esr(a, b, trim: int = TRIM) -> float:
    a, b = np.asarray(a, np.float64)[trim:len(b) - trim], np.asarray(b, np.float64)[trim:len(b) - trim]
    return float(((a - b) ** 2).sum() / (b ** 2).sum())


@functools.lru_cache(maxsize=None)
def acceptance(name: str):
    """dict of the helper's own figures on a pair: the line, its largest position error over the file, the ESR of
    estimate-then-warp against the true wet, the ESR of the constant median lag (K19's reduction), the warped wet (fp64)."""
    drift, offset, pol, _ = PAIRS[name]
    dry, wet = source()
    rec = recorded(name)
    c, l, f, r = probes(dry, rec)
    line = fit_lag_line(c, l + f, r)
    n = np.arange(L, dtype=np.float64)
    pos_err = float(np.abs((line.offset + line.drift * n) - (offset + drift * n)).max())
    warped = rows(rec, line.offset, line.drift, n_out=L, sign=line.polarity)
    lag = sorted(int(v) for v in l)[(len(l) - 1) // 2]           # datasets.reduce_probe_lags: the lower median
    const = pair_align64.shift64(np.pad(rec, (0, max(0, L - len(rec))))[None, :], [lag], [float(np.sum(r))])[0][:L]
    warped.setflags(write=False)
    return {"line": line, "pos_err": pos_err, "esr": esr(warped, wet), "esr_const": esr(const, wet), "warped": warped,
            "probes": (c, l, f, r), "median_lag": lag}

"""numpy fp64 restatement of csrc/fx_params.hip (DESIGN K16), written from the definition: the map of the learned effect
parameters onto their ranges, its derivative with respect to raw, the per-row constants ``mx_fx_params_expand`` writes and
the reduction of ``mx_fx_params_grad``.  No torch, no kernel code."""
import numpy as np

KINDS = ("flanger", "chorus", "phaser", "tremolo", "dry")
SLOTS = ("lfo_scale", "min_delay", "feedback", "depth", "mix", "centre_frequency_hz")
NAME_SLOT = {"width": "lfo_scale", "min_delay_width": "min_delay", "feedback": "feedback", "depth": "depth", "mix": "mix",
             "centre_frequency_hz": "centre_frequency_hz"}


def sigmoid(z):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def value(raw, lo, hi, is_log, gain=1.0):
    """The mapped values (fp64) of raw (P,): lo + (hi - lo) s, or exp(log lo + (log hi - log lo) s), s = sigmoid(gain raw)."""
    raw, lo, hi = (np.asarray(a, dtype=np.float64) for a in (raw, lo, hi))
    is_log = np.asarray(is_log, dtype=bool)
    s = sigmoid(gain * raw)
    lin = lo + (hi - lo) * s
    with np.errstate(invalid="ignore", divide="ignore"):
        l0 = np.log(np.where(is_log, lo, 1.0))
        l1 = np.log(np.where(is_log, hi, 1.0))
    return np.where(is_log, np.exp(l0 + (l1 - l0) * s), lin)


def dvalue_draw(raw, lo, hi, is_log, gain=1.0):
    """d value / d raw (fp64), analytically."""
    raw, lo, hi = (np.asarray(a, dtype=np.float64) for a in (raw, lo, hi))
    is_log = np.asarray(is_log, dtype=bool)
    s = sigmoid(gain * raw)
    ds = gain * s * (1.0 - s)
    with np.errstate(invalid="ignore", divide="ignore"):
        span = np.log(np.where(is_log, hi, 1.0)) - np.log(np.where(is_log, lo, 1.0))
    return np.where(is_log, value(raw, lo, hi, is_log, gain) * span * ds, (hi - lo) * ds)


def expand(raw, lo, hi, is_log, slot, kind, gain, row_kind, max_lfo_delay, max_min_delay):
    """{slot name: (values (B,) fp64, written (B,) bool)} for the six slots and "one_minus_mix": the fp64 value, NOT rounded
    (times the row's sample count for lfo_scale / min_delay; 1 - value for one_minus_mix), and which rows an entry covers."""
    v = value(raw, lo, hi, is_log, gain)
    row_kind = np.asarray(row_kind)
    B = row_kind.size
    out = {name: (np.zeros(B), np.zeros(B, dtype=bool)) for name in SLOTS + ("one_minus_mix",)}
    for e in range(len(v)):
        rows = row_kind == kind[e]
        name = SLOTS[slot[e]]
        scale = np.asarray(max_lfo_delay, dtype=np.float64) if name == "lfo_scale" else \
            np.asarray(max_min_delay, dtype=np.float64) if name == "min_delay" else np.ones(B)
        out[name][0][rows] = (v[e] * scale)[rows]
        out[name][1][rows] = True
        if name == "mix":
            out["one_minus_mix"][0][rows] = 1.0 - v[e]
            out["one_minus_mix"][1][rows] = True
    return out


def grad(grads, raw, lo, hi, is_log, slot, kind, gain, row_kind, max_lfo_delay, max_min_delay, scale=1.0):
    """(d_raw (P,) fp64, abs_terms (P,) fp64): scale * d loss / d raw from grads (6, B) fp64, and the sum of the absolute
    values of the terms of each entry's sum in the output's units (for the reduction's error bound)."""
    grads = np.asarray(grads, dtype=np.float64)
    row_kind = np.asarray(row_kind)
    dv = dvalue_draw(raw, lo, hi, is_log, gain)
    P = len(dv)
    out, mag = np.zeros(P), np.zeros(P)
    for e in range(P):
        rows = row_kind == kind[e]
        t = grads[slot[e]][rows]
        if SLOTS[slot[e]] == "lfo_scale":
            t = t * np.asarray(max_lfo_delay, dtype=np.float64)[rows]
        if SLOTS[slot[e]] == "min_delay":
            t = t * np.asarray(max_min_delay, dtype=np.float64)[rows]
        out[e] = np.sum(t) * dv[e] * scale
        mag[e] = np.sum(np.abs(t)) * abs(dv[e] * scale)
    return out, mag

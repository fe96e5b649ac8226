"""numpy fp64 restatement of csrc/fx_head.hip (DESIGN K17), written from the definition: the mean pool of the latent, the
linear layer, the map onto the parameters' ranges (``fx_params64.value`` / ``dvalue_draw``), the per-row constants
``mx_fx_head_fwd`` writes and the backward of ``mx_fx_head_bwd``, with the sums of absolute terms the error bounds of the
kernel tests need.  No torch, no kernel code."""
import numpy as np

from tests.helpers import fx_params64 as p64

SLOTS = p64.SLOTS


def pool(latent):
    """(pooled (B, C) fp64, abs_terms (B, C) = sum_w |latent|): the mean over the last axis."""
    latent = np.asarray(latent, dtype=np.float64)
    return latent.mean(-1), np.abs(latent).sum(-1)


def linear(pooled, weight, bias):
    """(raw (B, P) fp64, abs_terms (B, P) = |bias| + sum_c |weight pooled|)."""
    pooled, weight, bias = (np.asarray(a, dtype=np.float64) for a in (pooled, weight, bias))
    return bias[None, :] + pooled @ weight.T, np.abs(bias)[None, :] + np.abs(pooled) @ np.abs(weight).T


def values(raw_rows, lo, hi, is_log, gain=1.0):
    """The mapped values (B, P) fp64 of raw_rows (B, P)."""
    raw_rows = np.asarray(raw_rows, dtype=np.float64)
    return np.stack([p64.value(r, lo, hi, is_log, gain) for r in raw_rows])


def forward(latent, weight, bias, lo, hi, is_log, gain=1.0):
    """(pooled, raw, values), all fp64 and unrounded."""
    pooled, _ = pool(latent)
    raw, _ = linear(pooled, weight, bias)
    return pooled, raw, values(raw, lo, hi, is_log, gain)


def expand(vals, slot, kind, row_kind, max_lfo_delay, max_min_delay):
    """{slot name: (values (B,) fp64, written (B,) bool)} for the six slots and "one_minus_mix" from per-clip values (B, P):
    ``fx_params64.expand`` with a value per row."""
    vals = np.asarray(vals, dtype=np.float64)
    row_kind = np.asarray(row_kind)
    B = row_kind.size
    out = {name: (np.zeros(B), np.zeros(B, dtype=bool)) for name in SLOTS + ("one_minus_mix",)}
    for e in range(vals.shape[1]):
        rows = row_kind == kind[e]
        name = SLOTS[slot[e]]
        scale = np.asarray(max_lfo_delay, dtype=np.float64) if name == "lfo_scale" else \
            np.asarray(max_min_delay, dtype=np.float64) if name == "min_delay" else np.ones(B)
        out[name][0][rows] = (vals[:, e] * scale)[rows]
        out[name][1][rows] = True
        if name == "mix":
            out["one_minus_mix"][0][rows] = 1.0 - vals[rows, e]
            out["one_minus_mix"][1][rows] = True
    return out


def d_raw_rows(grads, raw_rows, lo, hi, is_log, slot, kind, gain, row_kind, max_lfo_delay, max_min_delay, scale=1.0):
    """d_raw (B, P) fp64: scale * grads[slot_e, b] * (the row's sample count where the slot has one) * d value / d raw at
    raw_rows[b, e] on the rows of the entry's kind, 0 elsewhere (grads may hold NaN there: it is not read)."""
    grads = np.asarray(grads, dtype=np.float64)
    raw_rows = np.asarray(raw_rows, dtype=np.float64)
    row_kind = np.asarray(row_kind)
    B, P = raw_rows.shape
    out = np.zeros((B, P))
    for e in range(P):
        dv = p64.dvalue_draw(raw_rows[:, e], np.full(B, lo[e]), np.full(B, hi[e]), np.full(B, bool(is_log[e])), gain)
        for b in np.nonzero(row_kind == kind[e])[0]:
            t = grads[slot[e], b]
            if SLOTS[slot[e]] == "lfo_scale":
                t = t * float(max_lfo_delay[b])
            if SLOTS[slot[e]] == "min_delay":
                t = t * float(max_min_delay[b])
            out[b, e] = scale * t * dv[b]
    return out


def backward(grads, raw_rows, pooled, weight, lo, hi, is_log, slot, kind, gain, row_kind, max_lfo_delay, max_min_delay, W,
             scale=1.0):
    """The backward from per-clip slot gradients (6, B): a dict with d_raw (B, P), d_bias (P,), d_weight (P, C), d_pooled
    (B, C), d_latent (B, C) (= d_pooled / W, the value of every w) and, under "abs_" + name, the sum of the absolute values
    of the terms of each of those sums (d_raw: the value's own magnitude)."""
    pooled, weight = np.asarray(pooled, dtype=np.float64), np.asarray(weight, dtype=np.float64)
    d = d_raw_rows(grads, raw_rows, lo, hi, is_log, slot, kind, gain, row_kind, max_lfo_delay, max_min_delay, scale)
    d_pooled, abs_pooled = d @ weight, np.abs(d) @ np.abs(weight)
    return {"d_raw": d, "abs_d_raw": np.abs(d),
            "d_bias": d.sum(0), "abs_d_bias": np.abs(d).sum(0),
            "d_weight": d.T @ pooled, "abs_d_weight": np.abs(d).T @ np.abs(pooled),
            "d_pooled": d_pooled, "abs_d_pooled": abs_pooled,
            "d_latent": d_pooled / W, "abs_d_latent": abs_pooled / W}

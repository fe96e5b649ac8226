"""The rate contour of a track (K25, mod_extraction_amd/csrc/rate_track_abi.h) restated in numpy fp64 on tests/helpers/lfo_fit64.py:
node costs per slice, the transition, the Viterbi path per shape, the choice of the shape, and K18's refinement per slice.

The transition is formed operation by operation in the header's order (numpy rounds every elementwise product, quotient and sum
on its own), so on equal node tables the path has the kernel's bits.  The node costs themselves come from ``lfo_fit64.objective``
(centred sums, numpy's summation order, a correctly rounded cosine): they differ from the kernel's by rounding.
"""
import numpy as np

from tests.helpers import lfo_fit64 as h
from tests.helpers import lfo_stitch64

F32 = np.float32


def window_starts(n, W, hop):
    """``file_eval.window_starts``: 0, hop, ... while the slice fits, and one right-aligned last slice if the end is uncovered."""
    starts = list(range(0, n - W + 1, hop))
    if starts[-1] != n - W:
        starts.append(n - W)
    return starts


def grid(W, sr, f_min, f_max, rate_div):
    """(f_min, f_max, sr, df, K) of a slice: ``lfo_fit64.grid_of`` on W points."""
    return h.grid_of(W, sr, f_min, f_max, rate_div)


def slice_nodes(ys, sr, sh, f_min, f_max, rate_div, J):
    """R / Syy of every coarse candidate c = k J + j of one slice (C,), or zeros for a constant slice."""
    W = len(ys)
    f_min, f_max, sr, df, K = grid(W, sr, f_min, f_max, rate_div)
    Syy = h.row_stats(ys)[2]
    if Syy == 0.0:
        return np.zeros(K * J)
    f, p = h._decode(np.arange(K * J), J, 0, f_min, df, 0.0, h.TWO_PI / J, f_min, f_max)
    f32, ph32 = h.candidate(sh, f, p, W, sr)
    return h.objective(ys, h.template(W, sr, sh, f32, ph32))["R"] / Syy


def node_table(y, sr, starts, W, f_min, f_max, mask, rate_div, J):
    """{shape id: (S, C) fp64} for the allowed shapes of one row."""
    y = np.asarray(y, dtype=F32)
    return {sh: np.stack([slice_nodes(y[s:s + W], sr, sh, f_min, f_max, rate_div, J) for s in starts])
            for sh in range(7) if (mask >> sh) & 1}


def rates(K, f_min, f_max, df):
    """f_k, as ``_decode`` forms them."""
    return np.clip(f_min + np.arange(K).astype(np.float64) * df, f_min, f_max)


def transition(sh, ka, ja, kb, jb, dstart, sr, fk, J, rate_weight, phase_weight):
    """tr(a, b) on broadcastable integer arrays: every operation rounded on its own, in the header's order."""
    q = 2 if sh in h.RECT else 1
    adv = ((0.5 * (fk[ka] + fk[kb])) * float(dstart)) / sr
    m = ((jb - ja) * q).astype(np.float64) / float(J) - adv
    m = m - np.rint(m)
    dk = (kb - ka).astype(np.float64)
    return rate_weight * (dk * dk) + phase_weight * (m * m)


def viterbi(node, sh, starts, sr, fk, J, D, rate_weight, phase_weight):
    """(total cost, path (S,) of candidate indices) through node (S, C): ties to the lowest source, the lowest end."""
    S, C = node.shape
    K = C // J
    V = node[0].copy()
    back = np.zeros((S, C), dtype=np.int64)
    kb = np.arange(K)[:, None, None]
    jb = np.arange(J)[None, :, None]
    ja = np.arange(J)[None, None, :]
    for s in range(1, S):
        Vk = V.reshape(K, J)
        best = np.full((K, J), np.inf)
        arg = np.zeros((K, J), dtype=np.int64)
        for dk in range(min(D, K - 1), -min(D, K - 1) - 1, -1):          # k_a = k_b - dk ascending
            ka = kb - dk
            ok = ((ka >= 0) & (ka < K))[:, 0, 0]
            kac = np.clip(ka, 0, K - 1)
            tr = transition(sh, kac, ja, kb, jb, starts[s] - starts[s - 1], sr, fk, J, rate_weight, phase_weight)
            cand = Vk[kac[:, 0, 0]][:, None, :] + tr                    # (K, J_b, J_a)
            j_min = np.argmin(cand, axis=2)                             # the first of equal minima: the lowest j_a
            v_min = np.take_along_axis(cand, j_min[:, :, None], axis=2)[:, :, 0]
            better = ok[:, None] & (v_min < best)
            best = np.where(better, v_min, best)
            arg = np.where(better, kac[:, :, 0] * J + j_min, arg)
        V = node[s] + best.reshape(C)
        back[s] = arg.reshape(C)
    end = int(np.argmin(V))
    path = np.zeros(S, dtype=np.int64)
    path[S - 1] = end
    for s in range(S - 1, 0, -1):
        path[s - 1] = back[s, path[s]]
    return float(V[end]), path


def path_cost(node, path, sh, starts, sr, fk, J, D, rate_weight, phase_weight):
    """The price of ANY path through node (S, C), summed as the recursion sums it; +inf if a step exceeds D bins."""
    V = float(node[0, path[0]])
    for s in range(1, len(path)):
        ka, ja, kb, jb = (np.asarray(v) for v in (path[s - 1] // J, path[s - 1] % J, path[s] // J, path[s] % J))
        if abs(int(kb) - int(ka)) > D:
            return np.inf
        tr = transition(sh, ka, ja, kb, jb, starts[s] - starts[s - 1], sr, fk, J, rate_weight, phase_weight)
        V = float(node[s, path[s]] + (V + tr))
    return V


def choose(nodes, starts, sr, fk, J, D, rate_weight, phase_weight):
    """(shape, path, per-shape costs (7,), +inf where not allowed) from a node table: least total cost, ties to the lowest id."""
    per = np.full(7, np.inf)
    best = None
    for sh in sorted(nodes):
        cost, path = viterbi(nodes[sh], sh, starts, sr, fk, J, D, rate_weight, phase_weight)
        per[sh] = cost
        if best is None or cost < best[0]:
            best = (cost, sh, path)
    return best[1], best[2], per


def refine_slice(ys, sr, sh, f_min, f_max, rate_div, J, L, c):
    """K18's rounds 1..L on one slice from coarse candidate c of shape sh: the slice's outputs before their fp32 rounding."""
    ys = np.asarray(ys, dtype=F32)
    W = len(ys)
    f_min, f_max, sr, df, K = grid(W, sr, f_min, f_max, rate_div)
    dphi = h.TWO_PI / J
    mean, _, Syy = h.row_stats(ys)
    f, p = h._decode(np.asarray([c]), J, 0, f_min, df, 0.0, dphi, f_min, f_max)
    f0, p0 = float(f[0]), float(p[0])
    f32, ph32 = h.candidate(sh, np.asarray([f0]), np.asarray([p0]), W, sr)
    if Syy == 0.0:
        return {"rate_hz": f32[0], "phase": ph32[0], "amp": 0.0, "offset": mean, "resid": 0.0}
    R0 = float(h.objective(ys, h.template(W, sr, sh, f32, ph32))["R"][0])
    for l in range(1, L + 1):
        scale = 1.0 / (1 << l)
        g = (5, 2, f0, df * scale, p0, dphi * scale)
        R, cc = h._stage(ys, sr, sh, 25, *g, f_min, f_max)
        if R < R0:
            R0 = R
            f, p = h._decode(cc, *g, f_min, f_max)
            f0, p0 = float(f), float(p)
    f32, ph32 = h.candidate(sh, np.asarray([f0]), np.asarray([p0]), W, sr)
    at = h.eval_at(ys, sr, sh, f32[0], ph32[0])
    return {"rate_hz": f32[0], "phase": ph32[0], "amp": at["a"], "offset": at["b"], "resid": R0 / Syy}


def fit(y, sr, starts, W, f_min=0.25, f_max=8.0, mask=h.DEFAULT_MASK, rate_div=4, J=32, L=4, D=2, rate_weight=0.002,
        phase_weight=1.0, nodes=None):
    """The rate contour of one row: dict with shape, path, grid_k, grid_j (S,), rate_hz, phase (fp32 by definition), amp, offset,
    resid (fp64, (S,)), cost, per_shape_cost (7,) and the node table.  ``nodes``: a node table to use in place of the row's own."""
    y = np.asarray(y, dtype=F32)
    starts = [int(s) for s in starts]
    f_lo, f_hi, srf, df, K = grid(W, sr, f_min, f_max, rate_div)
    fk = rates(K, f_lo, f_hi, df)
    if nodes is None:
        nodes = node_table(y, sr, starts, W, f_min, f_max, mask, rate_div, J)
    sh, path, per = choose(nodes, starts, srf, fk, J, D, rate_weight, phase_weight)
    sl = [refine_slice(y[s:s + W], sr, sh, f_min, f_max, rate_div, J, L, int(c)) for s, c in zip(starts, path)]
    out = {k: np.asarray([v[k] for v in sl]) for k in ("rate_hz", "phase", "amp", "offset", "resid")}
    out.update(shape=sh, path=path, grid_k=path // J, grid_j=path % J, cost=per[sh], per_shape_cost=per, nodes=nodes, fk=fk,
               sr=srf, starts=starts, W=W)
    return out


def templates(fit_, sr):
    """(S, W) fp32: ``modulations.synth_from_fit``'s formula on every slice."""
    return np.stack([h.synth({"shape": fit_["shape"], "rate_hz": r, "phase": p, "amp": a, "offset": o}, fit_["W"], sr)
                     for r, p, a, o in zip(fit_["rate_hz"], fit_["phase"], fit_["amp"], fit_["offset"])])


def stitched(fit_, sr, n):
    """The slices' templates joined by K22's taper at integer positions (n_f = N = W, n_t = L = n): (n,) fp64."""
    return lfo_stitch64.stitch(templates(fit_, sr), fit_["starts"], n, fit_["W"], n)[0]


def glide(n, sr, shape, f0, f1, amp=0.7, offset=0.1, noise=0.0, rng=None, wobble=0.0):
    """(noisy fp32 row, noise-free fp64 row, rate at every point): an LFO whose rate moves linearly from f0 to f1 over the row,
    its phase the running integral of the rate.  Shapes as ``lfo_value`` draws them, in fp64."""
    t = np.arange(1, n + 1) / sr
    f = f0 + (f1 - f0) * (t - t[0]) / (t[-1] - t[0]) + wobble * np.sin(2 * np.pi * 0.1 * t)
    cyc = np.cumsum(f) / sr                                     # cycles
    arg = 2 * np.pi * cyc
    if shape == "cos":
        v = (np.cos(arg + np.pi) + 1.0) * 0.5
    elif shape == "rect_cos":
        v = np.abs(np.cos(0.5 * arg + 0.5 * np.pi))
    elif shape == "inv_rect_cos":
        v = 1.0 - np.abs(np.cos(0.5 * arg))
    else:
        saw = np.mod(cyc, 1.0)
        v = {"saw": saw, "rsaw": 1.0 - saw, "tri": np.where(2 * saw > 1, 2 - 2 * saw, 2 * saw)}[shape]
    clean = offset + amp * v
    noisy = clean + (rng.normal(0.0, noise, n) if noise > 0.0 else 0.0)
    return noisy.astype(F32), clean, f

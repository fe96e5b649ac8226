"""Independent references of the oldest kernel family: LFO synthesis and resampling (lfo.hip, K1), the corner bookkeeping
(corners.hip, K9) and mx_lfo_loss (head_loss.hip).  numpy only -- no torch, no device.  tests/test_lfo_units64.py holds every
function here against oracle.modulations / oracle.util / oracle.losses; tests/test_gpu_lfo_units.py holds the kernels against
these.

Two kinds of arithmetic, kept apart:

* what the kernels document as IEEE basic operations in fp32 (add, sub, mul, div, fmod, floor, min, int conversion) is restated
  in numpy fp32 and is EXACT: the phase argument, the saw / triangle bookkeeping, the interpolation taps, the corner maps, the
  stretch, the validity rule.  The tests compare these with ==;
* everything transcendental or summed (cos, pow, the interpolation sum, the stretch gradient, the loss) is evaluated in fp64
  from those fp32 quantities.

Disputed line, settled by the reference project (mod_extraction/lightning.py:48-52):
        if weighting > 0:
            if loss is None:
                loss = weighting * loss_value
            else:
                loss += weighting * loss_value
  The trained quantity is that `loss`, so a term whose weight is zero or negative is absent from d loss / d y_hat as well as from
  the total.  mx_lfo_loss used to add such a term to the gradient with its (negative) weight; ``lfo_loss64`` states the
  reference's rule.
"""
import math

import numpy as np

f32, f64 = np.float32, np.float64
SHAPES = ("cos", "rect_cos", "inv_rect_cos", "tri", "saw", "rsaw", "sqr")          # the LFO_* codes of lfo_common.h, in order
COS, RECT_COS, INV_RECT_COS, TRI, SAW, RSAW, SQR = range(7)
TWO_PI_F, PI_F, HALF_PI_F = f32(6.283185307179586), f32(3.141592653589793), f32(1.5707963267948966)


def _code(shape):
    return SHAPES.index(shape) if isinstance(shape, str) else int(shape)


# ==== K1: synthesis ============================================================================================================
def lfo_arg32(k, start, freq, phase, shape, sr):
    """The fp32 phase argument of point(s) ``k`` as lfo_common.h documents it: the rectified cosines run at half rate and half
    phase (exact halvings), step = fl32(fl32(2 pi f) / sr), arg = fl32(fl32(fl64(k + 1 + start) fl64(step)) + fl32(phase))."""
    sh = _code(shape)
    f, ph = f32(freq), f32(phase)
    if sh in (RECT_COS, INV_RECT_COS):
        f, ph = f32(f * f32(0.5)), f32(ph * f32(0.5))
    step = f32(f32(TWO_PI_F * f) / f32(sr))
    run = ((np.asarray(k, np.int64) + 1 + int(start)).astype(f64) * f64(step)).astype(f32)
    return (run + ph).astype(f32)


def _saw32(arg32):
    """(arg mod 2 pi) and saw = fl32(that / 2 pi): fmod is exact, torch.remainder's sign rule, one fp32 division."""
    m = np.fmod(np.asarray(arg32, f32), TWO_PI_F).astype(f32)
    m = np.where((m != 0) & (m < 0), (m + TWO_PI_F).astype(f32), m).astype(f32)
    return m, (m / TWO_PI_F).astype(f32)


def _phase_shape32(arg32, sh):
    m, saw = _saw32(arg32)
    if sh == SAW:
        return m, saw
    if sh == RSAW:
        return m, (f32(1.0) - saw).astype(f32)
    tri = (f32(2.0) * saw).astype(f32)
    return m, np.where(tri > f32(1.0), (f32(2.0) - tri).astype(f32), tri).astype(f32)


def lfo_bits32(arg32, shape, exp):
    """saw / rsaw / tri at exponent 1, 2 or 3: only IEEE basic fp32 operations (v, fl32(v v), fl32(fl32(v v) v)), so the fp32
    result is determined -- the kernel must produce these bits."""
    sh = _code(shape)
    assert sh in (TRI, SAW, RSAW) and exp in (1.0, 2.0, 3.0)
    v = _phase_shape32(arg32, sh)[1]
    if exp == 2.0:
        return (v * v).astype(f32)
    if exp == 3.0:
        return ((v * v).astype(f32) * v).astype(f32)
    return v


def lfo_value64(arg32, shape, exp=1.0):
    """(value, margin): the shape function and the power in fp64 from the fp32 argument.  The argument offsets (+ pi, + pi / 2)
    are the kernel's fp32 additions -- at arg ~ 1e5 one fp32 ulp of the argument is 0.008 rad, so that rounding is part of the
    function, not of its error -- and so are the saw's exact fmod and its fp32 division; cos, the affine maps of the cosine
    family and the power are fp64.
    margin: how far the point is from a decision that fp32 may legitimately take either way -- |cos| for sqr, 1 for the other
    cosines; for saw / rsaw / tri the distance of arg mod 2 pi from the jump (0 and 2 pi), for tri also from the fold (pi)."""
    sh = _code(shape)
    a = np.asarray(arg32, f32)
    margin = np.ones(a.shape, f64)
    if sh == COS:
        v = (np.cos((a + PI_F).astype(f32).astype(f64)) + 1.0) * 0.5
    elif sh == RECT_COS:
        v = np.abs(np.cos((a + HALF_PI_F).astype(f32).astype(f64)))
    elif sh == INV_RECT_COS:
        v = 1.0 - np.abs(np.cos(a.astype(f64)))
    elif sh == SQR:
        c = np.cos((a + PI_F).astype(f32).astype(f64))
        v = (np.sign(c) + 1.0) * 0.5
        margin = np.abs(c)
    else:
        m, v32 = _phase_shape32(a, sh)
        v = v32.astype(f64)
        m = m.astype(f64)
        margin = np.minimum(m, 2.0 * math.pi - m)
        if sh == TRI:
            margin = np.minimum(margin, np.abs(m - math.pi))
    if exp != 1.0:
        v = np.power(np.maximum(v, 0.0), f64(f32(exp)))
    return v, margin


def lfo_synth64(freq, phase, shape, exp, start, n_src, n_out, sr):
    """One launch of mx_lfo_synth: per-row arrays (shape / exp / start may be None as the null pointers are) -> (value (B, n_out)
    fp64, margin (B, n_out), arg32 (B, n_src)).  n_out != n_src: the two taps of interp_taps32, combined in fp64; the margin of
    a resampled point is the smaller one of the taps that carry weight."""
    B = len(freq)
    val, mar, args = np.zeros((B, n_out)), np.zeros((B, n_out)), np.zeros((B, n_src), f32)
    i0, i1, lam0, lam1 = interp_taps32(n_src, n_out)
    for b in range(B):
        sh = COS if shape is None else int(shape[b])
        e = 1.0 if exp is None else float(exp[b])
        st = 0 if start is None else int(start[b])
        args[b] = lfo_arg32(np.arange(n_src), st, freq[b], phase[b], sh, sr)
        v, m = lfo_value64(args[b], sh, e)
        if n_out == n_src:
            val[b], mar[b] = v, m
        else:
            val[b] = lam0.astype(f64) * v[i0] + lam1.astype(f64) * v[i1]
            mar[b] = np.minimum(np.where(lam0 != 0, m[i0], np.inf), np.where(lam1 != 0, m[i1], np.inf))
    return val, mar, args


# ==== util.py:15-29: align_corners linear resampling ===========================================================================
def interp_taps32(n_in, n_out):
    """(i0, i1, lam0, lam1) as interp_tap computes them: real = fl32(scale j) with scale = fl32(fl32(n_in - 1) / fl32(n_out - 1))
    (0 for one output), i0 = min(trunc(real), n_in - 1), lam1 = clamp(fl32(real - i0), 0, 1), lam0 = fl32(1 - lam1)."""
    scale = f32(f32(n_in - 1) / f32(n_out - 1)) if n_out > 1 else f32(0.0)
    real = (scale * np.arange(n_out).astype(f32)).astype(f32)
    i0 = np.minimum(np.trunc(real).astype(np.int64), n_in - 1)
    lam1 = np.minimum(np.maximum((real - i0.astype(f32)).astype(f32), f32(0.0)), f32(1.0)).astype(f32)
    i1 = np.where(i0 < n_in - 1, i0 + 1, i0)
    return i0, i1, (f32(1.0) - lam1).astype(f32), lam1


def interp64(x, n_in, n_out):
    """lam0 x[i0] + lam1 x[i1] in fp64, rows (R, n_in) -> (R, n_out)."""
    x = np.asarray(x, f64)
    assert x.shape[-1] == n_in
    i0, i1, lam0, lam1 = interp_taps32(n_in, n_out)
    return lam0.astype(f64) * x[..., i0] + lam1.astype(f64) * x[..., i1]


def interp_bwd64(dy_window, n_in, n_out, j0):
    """The transposed taps applied to a window dy (R, j_len) = d loss / d y[:, j0 : j0 + j_len], summed in fp64 -> (R, n_in)."""
    dy = np.asarray(dy_window, f64)
    i0, i1, lam0, lam1 = interp_taps32(n_in, n_out)
    js = j0 + np.arange(dy.shape[-1])
    dx = np.zeros((n_in,) + dy.shape[:-1], f64)                              # (n_in, R): np.add.at sums repeated indices
    np.add.at(dx, i0[js], (lam0[js].astype(f64) * dy).T)
    np.add.at(dx, i1[js], (lam1[js].astype(f64) * dy).T)
    return np.ascontiguousarray(dx.T)


# ==== K9: corners ==============================================================================================================
def smoothen_ref(x, k):
    """Left-to-right fp32 sum of k frames, one fp32 division (modulations.py:359-363 as corners.hip evaluates it)."""
    x = np.asarray(x, f32)
    n_out = x.shape[-1] - k + 1
    acc = np.zeros(x.shape[:-1] + (n_out,), f32)
    for j in range(k):
        acc = (acc + x[..., j:j + n_out]).astype(f32)
    return (acc / f32(k)).astype(f32)


def corners_ref(m):
    """(top, bot) fp32 maps of rows (R, n), zero at both ends: at interior i with d_l = m[i] - m[i-1], d_r = m[i+1] - m[i]
    top = -floor(max(d_l, 0) (d_r + 1e-16)), bot = -floor(min(d_l, 0) (d_r + 1e-16)), every operation rounded to fp32.
    (A plateau after a fall is a bottom corner through the nudge, a plateau after a rise is no top corner; a product beyond 1
    gives a map value beyond 1, of either sign.)"""
    m = np.asarray(m, f32)
    assert m.ndim == 2 and m.shape[1] >= 3
    d = (m[:, 1:] - m[:, :-1]).astype(f32)
    d_l, nudged = d[:, :-1], (d[:, 1:] + f32(1e-16)).astype(f32)
    top, bot = np.zeros_like(m), np.zeros_like(m)
    top[:, 1:-1] = -np.floor((np.maximum(d_l, f32(0.0)) * nudged).astype(f32))
    bot[:, 1:-1] = -np.floor((np.minimum(d_l, f32(0.0)) * nudged).astype(f32))
    return top + f32(0.0), bot + f32(0.0)                                    # -0 -> +0, as the reference's integer maps have it


def _count(c):
    """The reference's t.sum() over a row: an fp32 sum of small integers, exact in any order."""
    return f32(np.asarray(c, f64).sum())


def stretch_ref(m, max_n_corners):
    """modulations.py:260-307 without the smoothing, rows (R, n): anchors are the points whose map value is EXACTLY 1 (top ->
    target 1, bottom -> target 0) and the last sample (target: its own value); a row whose map values sum to more than
    max_n_corners is copied.  Per segment (p, i] with a target differing from the previous one: subtract the segment's minimum,
    multiply by gain = |previous target - target| / |m[p] - m[i]|, add target - (the segment's last value) -- fp32 throughout.
    Equal anchors give a gain that is not finite (the reference does the same division)."""
    m = np.asarray(m, f32)
    top, bot = corners_ref(m)
    out = m.copy()
    n = m.shape[1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for r in range(m.shape[0]):
            if f32(_count(top[r]) + _count(bot[r])) > f32(max_n_corners):
                continue
            row, o = m[r], out[r]
            prev_i, prev_t = 0, row[0]
            for i in range(1, n):
                if i == n - 1:
                    target = row[n - 1]
                elif top[r, i] == 1:
                    target = f32(1.0)
                elif bot[r, i] == 1:
                    target = f32(0.0)
                else:
                    continue
                if prev_t != target:
                    gain = f32(np.abs(f32(prev_t - target)) / np.abs(f32(row[prev_i] - row[i])))
                    seg = o[prev_i + 1:i + 1]
                    seg[:] = ((seg - seg.min()).astype(f32) * gain).astype(f32)
                    seg[:] = (seg + f32(target - seg[-1])).astype(f32)
                prev_i, prev_t = i, target
    return out


def valid_ref(m, min_top, max_top, min_bot, max_bot, min_gap):
    """modulations.py:311-343 per row -> int32 0 / 1: the map sums within [min, max] for tops and for bottoms, and consecutive
    like corners (map value exactly 1) at least min_gap frames apart."""
    top, bot = corners_ref(m)
    out = np.zeros(top.shape[0], np.int32)
    for r in range(top.shape[0]):
        n_top, n_bot = _count(top[r]), _count(bot[r])
        ok = not (n_top < min_top or n_bot < min_bot or n_top > max_top or n_bot > max_bot)
        for c in (top[r], bot[r]):
            idx = np.nonzero(c == 1)[0]
            if idx.size > 1 and int(np.diff(idx).min()) < min_gap:
                ok = False
        out[r] = int(ok)
    return out


def stretch_gain_finite(m, max_n_corners):
    """Per row: True unless a stretched segment has equal anchors (gain = x / 0)."""
    with np.errstate(all="ignore"):
        return np.isfinite(stretch_ref(m, max_n_corners)).all(axis=1)


def stretch_passthrough(m, max_n_corners):
    """(R, n) bool: where d loss / d m is d loss / d out itself -- every element of a copied row; elsewhere everything outside
    the stretched segments (p, i] and their left anchors p (which receive the gain's gradient)."""
    m = np.asarray(m, f32)
    top, bot = corners_ref(m)
    keep = np.ones(m.shape, bool)
    n = m.shape[1]
    for r in range(m.shape[0]):
        if f32(_count(top[r]) + _count(bot[r])) > f32(max_n_corners):
            continue
        prev_i, prev_t = 0, m[r, 0]
        for i in range(1, n):
            if i == n - 1:
                target = m[r, n - 1]
            elif top[r, i] == 1:
                target = f32(1.0)
            elif bot[r, i] == 1:
                target = f32(0.0)
            else:
                continue
            if prev_t != target:
                keep[r, prev_i:i + 1] = False
            prev_i, prev_t = i, target
    return keep


def stretch_bwd64(m, g, max_n_corners):
    """d loss / d m for out = stretch(m) and g = d loss / d out, the closed form of stretch_corners_bwd_kernel's header in fp64.
    The anchors and targets are the discrete decisions of corners_ref (no gradient).  A stretched segment S = (p, i] is, in
    exact arithmetic, out_j = (m_j - m_i) gain + target with gain = |A - target| / |m_p - m_i|, A the previous target (the
    tensor m_0 for the first segment), target the tensor m_(n-1) for the last.  With s1 = sum_S g_j, s2 = sum_S g_j (m_j - m_i):
        dm_j = g_j gain (j in S);  dm_i -= gain s1;  dH = -s2 gain / |m_p - m_i|:  dm_p += dH sign(m_p - m_i), dm_i -= the same;
        dW = s2 / |m_p - m_i|:  first segment dm_0 += dW sign(A - target);  last segment dm_i += s1 - dW sign(A - target).
    Everything else passes g through."""
    m32 = np.asarray(m, f32)
    top, bot = corners_ref(m32)
    m64, g = m32.astype(f64), np.asarray(g, f64)
    d = g.copy()
    n = m32.shape[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        for r in range(m32.shape[0]):
            if f32(_count(top[r]) + _count(bot[r])) > f32(max_n_corners):
                continue
            row, G, D = m64[r], g[r], d[r]
            prev_i, prev_t = 0, row[0]
            for i in range(1, n):
                last = i == n - 1
                if last:
                    target = row[n - 1]
                elif top[r, i] == 1:
                    target = 1.0
                elif bot[r, i] == 1:
                    target = 0.0
                else:
                    continue
                if prev_t != target:
                    dm, e = row[prev_i] - row[i], prev_t - target
                    have, want = abs(dm), abs(e)
                    gain = want / have
                    seg = slice(prev_i + 1, i + 1)
                    s1, s2 = G[seg].sum(), (G[seg] * (row[seg] - row[i])).sum()
                    D[seg] = G[seg] * gain
                    dh, dw = -s2 * gain / have, s2 / have
                    D[i] -= gain * s1 + dh * np.sign(dm)
                    D[prev_i] += dh * np.sign(dm)
                    if prev_i == 0:
                        D[0] += dw * np.sign(e)
                    if last:
                        D[i] += s1 - dw * np.sign(e)
                prev_i, prev_t = i, target
    return d


# ==== mx_lfo_loss ==============================================================================================================
def lfo_loss64(y_hat, y, w):
    """w = (w_l1, w_fdl1, w_sdl1, w_mse).  From the fp32 inputs, in fp64: the four means (|e| over B n, |d1 e| over B (n - 2),
    |d2 e| over B (n - 4), e^2 over B n; d1 x[i] = (x[i+2] - x[i]) / 2, d2 = d1 d1), total = the sum over w_k > 0 of w_k term_k
    (lightning.py:48-52, see the module docstring), grad = d total / d y_hat with sign(0) = 0, and per element the decision
    margin: the smallest |e|, |d1 e|, |d2 e| among the terms with a non-zero weight that touch the element (inf if none)."""
    a, t = np.asarray(y_hat, f32).astype(f64), np.asarray(y, f32).astype(f64)
    B, n = a.shape
    e = a - t
    d1 = lambda x: (x[:, 2:] - x[:, :-2]) / 2.0
    e1 = d1(a) - d1(t) if n > 2 else np.zeros((B, 0))
    e2 = d1(d1(a)) - d1(d1(t)) if n > 4 else np.zeros((B, 0))
    terms = np.array([np.abs(e).mean(), np.abs(e1).mean() if n > 2 else 0.0, np.abs(e2).mean() if n > 4 else 0.0, (e * e).mean()])
    total = float(sum(f64(f32(wk)) * tk for wk, tk in zip(w, terms) if wk > 0))
    grad, margin = np.zeros((B, n)), np.full((B, n), np.inf)
    w_l1, w_fd, w_sd, w_mse = (float(f32(v)) for v in w)
    if w_l1 > 0:
        grad += w_l1 / (B * n) * np.sign(e)
    if w_mse > 0:
        grad += 2.0 * w_mse / (B * n) * e
    if w_fd > 0 and n > 2:
        s = np.sign(e1) * (w_fd / (B * (n - 2)) * 0.5)
        grad[:, 2:] += s
        grad[:, :-2] -= s
    if w_sd > 0 and n > 4:
        s = np.sign(e2) * (w_sd / (B * (n - 4)) * 0.25)
        grad[:, 4:] += s
        grad[:, 2:-2] -= 2.0 * s
        grad[:, :-4] += s
    if w_l1 != 0:
        margin = np.minimum(margin, np.abs(e))
    if w_fd != 0 and n > 2:
        margin[:, 2:] = np.minimum(margin[:, 2:], np.abs(e1))
        margin[:, :-2] = np.minimum(margin[:, :-2], np.abs(e1))
    if w_sd != 0 and n > 4:
        for lo in (0, 2, 4):
            margin[:, lo:n - 4 + lo] = np.minimum(margin[:, lo:n - 4 + lo], np.abs(e2))
    return {"terms": terms, "total": total, "grad": grad, "margin": margin}


# ==== rows with a known corner structure =======================================================================================
GRID = 64                                                # values are k / 64: every difference of two of them is exact in fp32


def _map_values(steps):
    """The corner maps of a row given by its integer increments (in 1 / 64), by integer arithmetic alone -- the 'known'
    structure, written without any floating point: l = step into the point, r = step out of it;
    rising (l > 0):  r < 0 -> ceil(|l r| / 4096);  r == 0 -> 0 (the nudge: floor of a tiny positive);  r > 0 -> -floor(l r / 4096)
    falling (l < 0): r > 0 -> ceil(|l r| / 4096);  r == 0 -> 1 (floor of a tiny negative);             r < 0 -> -floor(l r / 4096)
    (1e-16 is far below half an ulp of any non-zero step, and |l r| < 2^24 keeps the fp32 product exact)."""
    n = len(steps) + 1
    top, bot = [0] * n, [0] * n
    for i in range(1, n - 1):
        l, r = steps[i - 1], steps[i]
        assert abs(l * r) < 2 ** 24
        mag = -((-abs(l * r)) // (GRID * GRID)) if l * r < 0 else -((l * r) // (GRID * GRID))
        if l > 0:
            top[i] = 0 if r == 0 else mag
        elif l < 0:
            bot[i] = 1 if r == 0 else mag
    return top, bot


def row_from_steps(steps, scale=1):
    """-> dict(row fp32 (n,), tops, bots: the indices whose map value is exactly 1, n_top, n_bot: the map sums, steps)."""
    steps = [int(s) * scale for s in steps]
    v = np.concatenate([[0], np.cumsum(steps)])
    row = ((v - v.min()).astype(f64) / GRID).astype(f32)
    top, bot = _map_values(steps)
    return {"row": row, "tops": [i for i, c in enumerate(top) if c == 1], "bots": [i for i, c in enumerate(bot) if c == 1],
            "n_top": sum(top), "n_bot": sum(bot), "steps": steps}


def zigzag(n, corners, first_up=True, slope=1, plateau=(), steep=None, scale=1):
    """A row of n samples with straight segments of +-slope / 64 per sample that turn at the interior indices ``corners``
    (ascending; the first segment rises if ``first_up``).  plateau: {corner index: w} holds the corner's value for w (2 or 3)
    equal samples before turning; steep: {corner index: s} makes the one step on either side of that corner s / 64."""
    steps, up, plateau, steep = [], first_up, dict(plateau), dict(steep or {})
    bounds = [0] + list(corners) + [n - 1]
    assert all(b > a for a, b in zip(bounds, bounds[1:])), bounds
    for a, b in zip(bounds, bounds[1:]):
        seg = [slope if up else -slope] * (b - a)
        if a in steep:
            seg[0] = steep[a] if up else -steep[a]
        if b in steep:
            seg[-1] = steep[b] if up else -steep[b]
        w = plateau.get(a, 1)
        assert w - 1 < len(seg)
        seg[:w - 1] = [0] * (w - 1)
        steps += seg
        up = not up
    return row_from_steps(steps, scale)


def _steep_for(value):
    """The step s with ceil(s s / 4096) == value: a single corner whose map value is ``value``."""
    s = 1
    while -((-s * s) // (GRID * GRID)) < value:
        s += 1
    assert -((-s * s) // (GRID * GRID)) == value
    return s


def counted_row(n, c_top, c_bot, gap=None):
    """A row whose top map sums to c_top and whose bottom map sums to c_bot (1 <= both <= 8).  Within one of each other the
    corners simply alternate.  More bottoms than that: the surplus tops are plateaus, which the rule does not see.  More tops:
    the only way the rule allows is a corner whose map value exceeds 1 (the count is the sum of the map), so the first top is
    made steep enough to carry the surplus.  gap: the spacing of like corners (default: spread over the row)."""
    assert 1 <= c_top <= 8 and 1 <= c_bot <= 8
    if abs(c_top - c_bot) <= 1:
        k, first_up = c_top + c_bot, c_top >= c_bot
    elif c_bot > c_top:
        k, first_up = 2 * c_bot - 1, False
    else:
        k, first_up = 2 * c_bot + 1, True
    half = gap // 2 if gap else max(2, (n - 1) // (k + 1))
    other = gap - half if gap else half
    spacing = [half if j % 2 == 0 else other for j in range(k - 1)]
    pos = list(np.cumsum([max(2, (n - 1 - sum(spacing)) // 2)] + spacing))
    assert pos[-1] <= n - 4, (n, c_top, c_bot, gap)
    plateau, steep = {}, {}
    if c_bot > c_top + 1:
        for j in range(1, k, 2)[c_top:]:                                     # the tops beyond the first c_top: hidden
            plateau[pos[j]] = 2
    elif c_top > c_bot + 1:
        steep[pos[0]] = _steep_for(c_top - c_bot)
    d = zigzag(n, pos, first_up, plateau=plateau, steep=steep)
    assert (d["n_top"], d["n_bot"]) == (c_top, c_bot), (d["n_top"], d["n_bot"], c_top, c_bot)
    return d


def designed_rows(n):
    """name -> dict(row, tops, bots, n_top, n_bot, steps) for every designed case that fits n samples.  Each dict also says
    ``gap``: the smallest spacing of like corners (None with fewer than two of either kind)."""
    out = {}

    def add(name, d):
        gaps = [b - a for idx in (d["tops"], d["bots"]) for a, b in zip(idx, idx[1:])]
        d["gap"] = min(gaps) if gaps else None
        out[name] = d

    add("monotone", zigzag(n, []))
    add("one_top", zigzag(n, [n // 2]))
    add("one_bottom", zigzag(n, [n // 2], first_up=False))
    if n >= 9:
        for k in (2, 3, 6, 7):                                               # exactly max_n_corners = 2, 6 corners and one more
            pos = [1 + j * ((n - 2) // k) for j in range(k)]
            add(f"alt{k}", zigzag(n, pos))
            add(f"alt{k}_down", zigzag(n, pos, first_up=False))
        add("plateau2_top_and_bottom", zigzag(n, [2, 5], plateau={2: 2, 5: 2}))
        # m[0] == m[3] behind a plateau the rule does not see; 3 is a bottom, m[0] != 0: the first segment's gain is x / 0
        add("equal_anchors", row_from_steps([1, 0, -1, 1] + [-1] * (n - 5)))
    if n >= 40:
        for k in (16, 17):
            pos = [2 + j * ((n - 4) // k) for j in range(k)]
            add(f"alt{k}", zigzag(n, pos))
        add("plateau3_top_and_bottom", zigzag(n, [n // 4, n // 2, 3 * n // 4], plateau={n // 4: 3, n // 2: 3, 3 * n // 4: 2}))
        add("scaled3", zigzag(n, [n // 4, n // 2, 3 * n // 4], steep={n // 2: 40}, scale=3))     # 9 x 1600 / 4096 -> map value 4
        add("scaled3_base", zigzag(n, [n // 4, n // 2, 3 * n // 4], steep={n // 2: 40}))         # the same row unscaled: value 1
        # the last sample equals the last bottom behind an unseen plateau: the LAST segment's gain is x / 0
        add("equal_anchors_end", row_from_steps([1] * (n - 10) + [-1] * 2 + [1] * 3 + [0] + [-1] * 3))
        for c, cp in ((1, 1), (2, 2), (6, 6), (7, 7), (2, 3), (3, 2), (1, 6), (6, 1), (2, 6), (7, 6), (6, 7), (8, 1), (1, 8), (8, 8), (3, 3),
                      (2, 1)):
            add(f"count_{c}_{cp}", counted_row(n, c, cp))
        for g in (8, 9, 10):
            add(f"gap{g}_tops", counted_row(n, 2, 3, gap=g))                 # bottoms g apart too (three of them)
            add(f"gap{g}_two_tops_one_bottom", counted_row(n, 2, 1, gap=g))
    return out

"""The LFO fit (K18, include/modex_hip.h) restated in numpy: the definition the kernel implements, vectorised over candidates.

Templates are the fp32 values of ``lfo_value`` (csrc/lfo_common.h): rate, phase and phase step are rounded to fp32 as the
kernel rounds them and every fp32 operation of ``lfo_value`` is an fp32 numpy operation; only the cosine is taken in fp64 of
the fp32 argument and rounded once (the correctly rounded fp32 cosine; a device ``cosf`` may differ by an ulp).  Everything
else -- the candidate's (f, ph), the centred sums, a, b, R -- is fp64.
"""
import numpy as np

F32 = np.float32
TWO_PI = 6.283185307179586
PI = 3.141592653589793
TWO_PI_F = F32(6.283185307179586)
PI_F = F32(3.141592653589793)
HALF_PI_F = F32(1.5707963267948966)
SHAPES = ("cos", "rect_cos", "inv_rect_cos", "tri", "saw", "rsaw", "sqr")
SHAPE_IDS = {s: i for i, s in enumerate(SHAPES)}
RECT = (1, 2)
DEFAULT_MASK = 0x3F


def mask_of(names):
    m = 0
    for s in names:
        m |= 1 << SHAPE_IDS[s]
    return m


def lfo_step(sh, f32, ph32, sr):
    """lfo_step: (step, ph) in fp32, the rectified cosines at half rate and half phase."""
    f32, ph32 = np.asarray(f32, dtype=F32), np.asarray(ph32, dtype=F32)
    if sh in RECT:
        f32, ph32 = f32 * F32(0.5), ph32 * F32(0.5)
    return (TWO_PI_F * f32) / F32(sr), ph32


def _cos32(a):
    return np.cos(a.astype(np.float64)).astype(F32)


def lfo_values(n, step, ph, sh, start=0):
    """lfo_value(k, start, step, ph, sh, 1) for k < n: step, ph (C,) fp32 (as lfo_step returns them) -> (C, n) fp32."""
    step, ph = np.atleast_1d(np.asarray(step, dtype=F32)), np.atleast_1d(np.asarray(ph, dtype=F32))
    k1 = np.arange(1 + start, n + 1 + start, dtype=np.float64)
    run = (k1[None, :] * step.astype(np.float64)[:, None]).astype(F32)
    arg = run + ph[:, None]
    assert arg.dtype == F32
    if sh == 0:
        return (_cos32(arg + PI_F) + F32(1.0)) * F32(0.5)
    if sh == 1:
        return np.abs(_cos32(arg + HALF_PI_F))
    if sh == 2:
        return -np.abs(_cos32(arg)) + F32(1.0)
    if sh == 6:
        return (np.sign(_cos32(arg + PI_F)) + F32(1.0)) * F32(0.5)
    m = np.fmod(arg, TWO_PI_F)
    m = np.where((m != 0) & (m < 0), m + TWO_PI_F, m).astype(F32)
    saw = m / TWO_PI_F
    if sh == 4:
        return saw
    if sh == 5:
        return F32(1.0) - saw
    tri = F32(2.0) * saw
    return np.where(tri > 1, F32(2.0) - tri, tri).astype(F32)


def template(n, sr, sh, rate32, ph32, start=0):
    """What mx_lfo_synth writes for (rate, phase, shape, exp = 1, start): (C, n) fp32."""
    step, ph = lfo_step(sh, rate32, ph32, sr)
    return lfo_values(n, step, ph, sh, start)


def candidate(sh, f, phic, n, sr):
    """(fl32 rate, fl32 phase) of the candidates (f, phic), fp64 arrays (C,)."""
    f32 = np.asarray(f, dtype=np.float64).astype(F32)
    step, _ = lfo_step(sh, f32, np.zeros_like(f32), sr)
    p = np.fmod(np.asarray(phic, dtype=np.float64) - step.astype(np.float64) * (0.5 * (n + 1)), TWO_PI)
    p = np.where(p < 0, p + TWO_PI, p)
    if sh in RECT:
        p = 2.0 * np.fmod(p, PI)
    ph32 = p.astype(F32)
    ph32[ph32 >= TWO_PI_F] = F32(0.0)
    return f32, ph32


def row_stats(y):
    y64 = np.asarray(y, dtype=F32).astype(np.float64)
    mean = float(y64.mean())
    yc = y64 - mean
    return mean, yc, float((yc * yc).sum())


def objective(y, t):
    """y (n,) fp32, t (C, n) fp32 -> dict of fp64 (C,) arrays R, a, b and the scalars Syy, mean."""
    mean, yc, Syy = row_stats(y)
    t64 = np.atleast_2d(t).astype(np.float64)
    mt = t64.mean(axis=1)
    tc = t64 - mt[:, None]
    Stt, Sty = (tc * tc).sum(axis=1), (tc * yc[None, :]).sum(axis=1)
    ok = (Stt > 0) & (Sty > 0)
    a = np.where(ok, Sty / np.where(Stt > 0, Stt, 1.0), 0.0)
    return {"R": Syy - a * Sty, "a": a, "b": mean - a * mt, "Syy": Syy, "mean": mean}


def eval_at(y, sr, sh, rate32, ph32):
    """The objective at one fp32 (shape, rate, phase): R, a, b, resid = R / Syy (fp64 floats)."""
    o = objective(y, template(len(y), sr, int(sh), F32(rate32), F32(ph32)))
    return {"R": float(o["R"][0]), "a": float(o["a"][0]), "b": float(o["b"][0]), "Syy": o["Syy"],
            "resid": float(o["R"][0] / o["Syy"]) if o["Syy"] > 0 else 0.0}


def _decode(c, width, off, fbase, fstep, pbase, pstep, f_min, f_max):
    c = np.asarray(c)
    ki, ji = c // width, c % width
    f = np.clip(fbase + (ki - off).astype(np.float64) * fstep, f_min, f_max)
    p = np.fmod(pbase + (ji - off).astype(np.float64) * pstep, TWO_PI)
    return f, np.where(p < 0, p + TWO_PI, p)


def _stage(y, sr, sh, ncand, *grid, chunk=1 << 21):
    """argmin of R over the candidates 0..ncand of a stage, ties to the lowest index: (R, c)."""
    n = len(y)
    best_R, best_c = np.inf, -1
    per = max(1, chunk // n)
    for lo in range(0, ncand, per):
        c = np.arange(lo, min(ncand, lo + per))
        f, p = _decode(c, *grid)
        f32, ph32 = candidate(sh, f, p, n, sr)
        R = objective(y, template(n, sr, sh, f32, ph32))["R"]
        i = int(np.argmin(R))                                   # the first of equal minima
        if R[i] < best_R:
            best_R, best_c = float(R[i]), int(c[i])
    return best_R, best_c


def grid_of(n, sr, f_min, f_max, rate_div):
    """(f_min, f_max, sr as the fp32 the ABI takes, in fp64), df and K."""
    f_min, f_max, sr = float(F32(f_min)), float(F32(f_max)), float(F32(sr))
    df = 1.0 / (rate_div * (n / sr))
    return f_min, f_max, sr, df, int(np.floor((f_max - f_min) / df)) + 1


def fit_shape(y, sr, sh, f_min, f_max, rate_div=4, J=32, L=4):
    """Coarse grid and L refinement rounds of one shape: (R, f, phic), fp64."""
    n = len(y)
    f_min, f_max, sr, df, K = grid_of(n, sr, f_min, f_max, rate_div)
    dphi = TWO_PI / J
    R0, f0, p0 = np.inf, f_min, 0.0
    for l in range(L + 1):
        scale = 1.0 / (1 << l)
        grid = (J, 0, f_min, df * scale, 0.0, dphi * scale) if l == 0 else (5, 2, f0, df * scale, p0, dphi * scale)
        R, c = _stage(y, sr, sh, K * J if l == 0 else 25, *grid, f_min, f_max)
        if R < R0:
            R0 = R
            f, p = _decode(c, *grid, f_min, f_max)
            f0, p0 = float(f), float(p)
    return R0, f0, p0


def fit_row(y, sr, f_min=0.25, f_max=8.0, mask=DEFAULT_MASK, rate_div=4, J=32, L=4):
    """The fit of one row: dict with shape, rate_hz, phase, amp, offset, resid (the kernel's outputs before their fp32
    rounding, rate_hz and phase being fp32 by definition), per_shape (7,) R / Syy (+inf where not allowed), R and Syy."""
    y = np.asarray(y, dtype=F32)
    n = len(y)
    allowed = [s for s in range(7) if (mask >> s) & 1]
    assert allowed
    mean, _, Syy = row_stats(y)
    per = np.full(7, np.inf)
    if Syy == 0.0:
        per[allowed] = 0.0
        return {"shape": allowed[0], "rate_hz": F32(f_min), "phase": F32(0.0), "amp": 0.0, "offset": mean, "resid": 0.0,
                "per_shape": per, "R": 0.0, "Syy": 0.0}
    best = None
    for sh in allowed:
        R, f, p = fit_shape(y, sr, sh, f_min, f_max, rate_div, J, L)
        per[sh] = R / Syy
        if best is None or R < best[0]:
            best = (R, f, p, sh)
    R, f, p, sh = best
    f32, ph32 = candidate(sh, np.asarray([f]), np.asarray([p]), n, float(F32(sr)))
    at = eval_at(y, float(F32(sr)), sh, f32[0], ph32[0])
    return {"shape": sh, "rate_hz": f32[0], "phase": ph32[0], "amp": at["a"], "offset": at["b"], "resid": R / Syy,
            "per_shape": per, "R": R, "Syy": Syy}


def synth(fit, n, sr, start=0):
    """``modulations.synth_from_fit``'s formula on one row's fit, in fp32: offset + amp * template."""
    t = template(n, float(F32(sr)), int(fit["shape"]), F32(fit["rate_hz"]), F32(fit["phase"]), start)[0]
    return F32(fit["offset"]) + F32(fit["amp"]) * t


def make_row(n, sr, shape, rate_hz, phase, amp=0.7, offset=0.1, noise=0.0, rng=None):
    """offset + amp * template (+ Gaussian noise), fp32: a test row."""
    t = template(n, float(F32(sr)), SHAPE_IDS[shape], F32(rate_hz), F32(phase))[0].astype(np.float64)
    y = offset + amp * t
    if noise > 0.0:
        y = y + rng.normal(0.0, noise, n)
    return y.astype(F32)

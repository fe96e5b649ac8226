"""fp64 explicit adjoint of the phaser recurrence (oracle_ref.c:orc_phaser), TEST INFRASTRUCTURE ONLY.

Per sample n of the T processed samples, G the coefficient of its 4-sample group:
    out_0 = x[n] - last;  stage k = 0..5: d_k = out_k - s_k, v_k = G d_k, y_k = v_k + s_k, s_k' = v_k + y_k, out_(k+1) = 2 y_k - out_k
    last' = fb out_6;  m = mix out_6 + (1 - mix) x[n];  y[n] = clip(m, -1, 1)
    per group: pre = osc (depth / 2) + norm_centre, lfo = clip(pre, 0, 1), fc = 10^(lfo (log_max - log_min) + log_min),
               g = tan(pi fc / sr), G = g / (1 + g);  osc = 1 - 2 mod (external LFO) or sin(phase - pi) (built-in)
The coefficient chain is evaluated in fp64 from the fp32 osc and parameters; the two clip masks (-1 <= m <= 1 and
0 <= pre <= 1, both closed: aten's clamp rule) are taken from the fp32 forward, which this module also evaluates op for op
(``forward32``: bit-identical to oracle.fx.phaser_np).  Everything else is fp64.

x, dy: (B, T) -- every processed sample, a lead included (the caller puts zeros into dy there); osc (B, ceil(T / 4)) fp32;
params: dict of (B,) fp32 arrays depth, centre_frequency_hz, feedback, mix.
"""
import ctypes
import ctypes.util
import math

import numpy as np

F32 = np.float32
TWO_PI_F = F32(6.283185307179586476925286766559)
PI_F = F32(3.14159265358979323846)
PARAMS = ("depth", "centre_frequency_hz", "feedback", "mix")


def _libm_f32(name, n_args):
    """The host libm's float function, elementwise on fp32 arrays: the oracle calls sinf / powf / log10f, and a libm's
    float results are not always the correctly rounded ones, so 'op for op' means the same library."""
    fn = getattr(ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6"), name)
    fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float] * n_args
    uf = np.frompyfunc(lambda *a: fn(*[float(v) for v in a]), n_args, 1)
    return lambda *arrays: np.asarray(uf(*[np.asarray(a, F32) for a in arrays])).astype(F32)


sinf, powf, log10f = _libm_f32("sinf", 1), _libm_f32("powf", 2), _libm_f32("log10f", 1)


def log_range(sr):
    """(log_min, log_max) fp32 of the cut-off axis: 20 Hz .. min(20 kHz, 0.49 sr)."""
    fmax = F32(min(20000.0, 0.49 * sr))
    return F32(log10f(F32(20.0))), F32(log10f(fmax))


def builtin_osc(rate, n_groups, sr):
    """JUCE's oscillator: osc[g] = sin(phase_g - pi), phase advanced in fp32 by 2 pi rate / (sr / 4) with wrap at 2 pi, 0 at
    group 0.  Returns (osc (B, n_groups) fp32, phase (B, n_groups) fp32)."""
    rate = np.asarray(rate, F32)
    inc = (TWO_PI_F / F32(sr / 4.0)) * rate
    ph = np.zeros(rate.shape, F32)
    phases = np.empty((rate.size, n_groups), F32)
    for g in range(n_groups):
        phases[:, g] = ph
        ph = ph + inc
        while (ph >= TWO_PI_F).any():
            ph = np.where(ph >= TWO_PI_F, ph - TWO_PI_F, ph).astype(F32)
    osc = sinf((phases - PI_F).astype(F32))
    return osc, phases


def chain32(osc, depth, centre, sr):
    """The coefficient chain as the fp32 forward evaluates it: (pre, lfo, G), each (B, n_groups) fp32."""
    log_min, log_max = log_range(sr)
    span = log_max - log_min
    nc = ((log10f(np.asarray(centre, F32)) - log_min) / span).astype(F32)
    vol = (np.asarray(depth, F32) * F32(0.5)).astype(F32)
    pre = ((np.asarray(osc, F32) * vol[:, None]).astype(F32) + nc[:, None]).astype(F32)
    lfo = np.clip(pre, F32(0.0), F32(1.0))
    fc = powf(np.full(lfo.shape, 10.0, F32), ((lfo * span).astype(F32) + log_min).astype(F32))
    g = np.tan(math.pi * fc.astype(np.float64) / sr).astype(F32)
    return pre, lfo, (g / (F32(1.0) + g)).astype(F32)


def chain64(osc, depth, centre, sr, pre32=None):
    """fp64 chain; the clamp decisions are those of pre32 when given.  Returns dict pre, inside, lfo, fc, g, G, span."""
    log_min, log_max = (float(v) for v in log_range(sr))
    span = log_max - log_min
    depth, centre = np.asarray(depth, np.float64), np.asarray(centre, np.float64)
    nc = (np.log10(centre) - log_min) / span
    pre = np.asarray(osc, np.float64) * (depth[:, None] / 2.0) + nc[:, None]
    ref = pre if pre32 is None else pre32
    inside = (ref >= 0.0) & (ref <= 1.0)
    lfo = np.where(inside, pre, np.where(ref < 0.0, 0.0, 1.0))
    fc = 10.0 ** (lfo * span + log_min)
    g = np.tan(math.pi * fc / sr)
    return {"pre": pre, "inside": inside, "lfo": lfo, "fc": fc, "g": g, "G": g / (1.0 + g), "span": span}


def cascade(x, G, fb, mix, keep=False):
    """The recurrence in the dtype of x (fp32: op for op as oracle_ref.c; fp64).  x (B, T), G (B, n_groups), fb, mix (B,).
    Returns m (B, T) before the output clip and, if keep, d (B, T, 6) and out_6 (B, T)."""
    dt = x.dtype.type
    B, T = x.shape
    s = [np.zeros(B, x.dtype) for _ in range(6)]
    last = np.zeros(B, x.dtype)
    wet, dry = mix.astype(x.dtype), (dt(1.0) - mix.astype(x.dtype))
    fb = fb.astype(x.dtype)
    m = np.empty((B, T), x.dtype)
    d = np.empty((B, T, 6), x.dtype) if keep else None
    o6 = np.empty((B, T), x.dtype) if keep else None
    two = dt(2.0)
    for n in range(T):
        Gn = G[:, n >> 2]
        xin = x[:, n]
        out = xin - last
        for k in range(6):
            dk = out - s[k]
            if keep:
                d[:, n, k] = dk
            v = Gn * dk
            yk = v + s[k]
            s[k] = v + yk
            out = two * yk - out
        last = out * fb
        m[:, n] = out * wet + xin * dry
        if keep:
            o6[:, n] = out
    return (m, d, o6) if keep else m


def forward32(x, osc, params, sr):
    """The fp32 forward, op for op: dict y, m (B, T), pre, lfo, G (B, n_groups), all fp32."""
    x = np.ascontiguousarray(x, F32)
    pre, lfo, G = chain32(osc, params["depth"], params["centre_frequency_hz"], sr)
    m = cascade(x, G, np.asarray(params["feedback"], F32), np.asarray(params["mix"], F32))
    return {"y": np.clip(m, F32(-1.0), F32(1.0)), "m": m, "pre": pre, "lfo": lfo, "G": G}


def forward64(x, mod, depth, centre, fb, mix, sr):
    """Pure fp64 forward from mod (osc = 1 - 2 mod) with its own clip decisions (finite differences): y (B, T)."""
    ch = chain64(1.0 - 2.0 * np.asarray(mod, np.float64), depth, centre, sr)
    m = cascade(np.asarray(x, np.float64), ch["G"], np.asarray(fb, np.float64), np.asarray(mix, np.float64))
    return np.clip(m, -1.0, 1.0)


def phaser_adjoint64(x, osc, params, sr, dy, fwd32=None, pass_m=None):
    """Gradients of sum(dy * y): dx (B, T), dmod (B, n_groups) (with respect to mod = (1 - osc) / 2) and the per-clip depth,
    centre_frequency_hz, feedback, mix (B,), all fp64.  Also "fwd32" (forward32's dict), "pass_m" (B, T) and "inside"
    (B, n_groups): the two clip masks, and "y64".  pass_m overrides the output-clip decisions (diagnostics: the decisions
    another forward took)."""
    x32 = np.ascontiguousarray(x, F32)
    B, T = x32.shape
    ng = (T + 3) // 4
    osc = np.asarray(osc, F32)
    assert osc.shape == (B, ng)
    f32 = fwd32 if fwd32 is not None else forward32(x32, osc, params, sr)
    p = {k: np.asarray(params[k], F32).astype(np.float64) for k in PARAMS}
    ch = chain64(osc, p["depth"], p["centre_frequency_hz"], sr, pre32=f32["pre"])
    G = ch["G"]
    x64 = x32.astype(np.float64)
    m, d, o6 = cascade(x64, G, p["feedback"], p["mix"], keep=True)
    if pass_m is None:
        pass_m = (f32["m"] >= -1.0) & (f32["m"] <= 1.0)
    gm = np.where(pass_m, np.asarray(dy, np.float64), 0.0)
    fb, mix = p["feedback"], p["mix"]
    L = np.zeros((B, 7))
    dx = np.empty((B, T))
    dG = np.zeros((B, ng))
    d_fb = np.zeros(B)
    for n in range(T - 1, -1, -1):
        Gn = G[:, n >> 2]
        d_fb += L[:, 6] * o6[:, n]
        g_out = mix * gm[:, n] + fb * L[:, 6]
        acc = np.zeros(B)
        for k in range(5, -1, -1):
            gy = 2.0 * g_out + L[:, k]
            gv = L[:, k] + gy
            acc += gv * d[:, n, k]
            L[:, k] = gy - Gn * gv
            g_out = Gn * gv - g_out
        dG[:, n >> 2] += acc
        dx[:, n] = (1.0 - mix) * gm[:, n] + g_out
        L[:, 6] = -g_out
    g, fc, span = ch["g"], ch["fc"], ch["span"]
    dlfo = np.where(ch["inside"], dG / (1.0 + g) ** 2 * (math.pi / sr) * (1.0 + g * g) * fc * math.log(10.0) * span, 0.0)
    y64 = np.where(pass_m, m, np.sign(f32["m"]).astype(np.float64))
    return {"dx": dx, "dmod": -dlfo * p["depth"][:, None],
            "depth": (dlfo * osc.astype(np.float64) / 2.0).sum(1),
            "centre_frequency_hz": dlfo.sum(1) / (p["centre_frequency_hz"] * math.log(10.0) * span),
            "feedback": d_fb, "mix": (gm * (o6 - x64)).sum(1),
            "fwd32": f32, "pass_m": pass_m, "inside": ch["inside"], "y64": y64, "dG": dG}

"""fp64 explicit adjoint of the flanger / chorus loop (mod_extraction/fx.py:92-119), TEST INFRASTRUCTURE ONLY.

The gradient is the derivative of the reference forward restated without in-place writes: floor (so prev / next) has zero
derivative, the read fraction and % have derivative 1, clip passes the gradient on [-1, 1] inclusive, never-written slots
read 0 and gradient sent to them is dropped.  Slots and fractions are the fp32 values of the reference's bookkeeping
(the rounding sequence of oracle.fx.flanger_torch_loop); everything after them is evaluated in fp64.  The clip mask is
taken from the fp32 forward (the z the reference computes), which this module also evaluates, op for op in fp32.

x, mod, dy: (B, N) arrays; consts: dict of (B,) fp32 arrays lfo_scale, min_delay, feedback, depth, mix, one_minus_mix
(fx.derive_clip_constants); M: delay-line length.
"""
import numpy as np

F32 = np.float32


def bookkeeping(mod, consts, M):
    """fp32 slots of fx.py:95-103: write slot w (N,), prev / next (B, N) int64, fraction (B, N) fp32."""
    mod = np.asarray(mod, F32)
    B, N = mod.shape
    w = np.arange(N) % M
    delay = (consts["lfo_scale"].astype(F32)[:, None] * mod).astype(F32) + consts["min_delay"].astype(F32)[:, None]
    r = np.remainder((w[None, :].astype(F32) - delay.astype(F32)).astype(F32) + F32(M), F32(M)).astype(F32)
    lo = np.floor(r).astype(F32)
    frac = (r - lo).astype(F32)
    prev = lo.astype(np.int64)
    nxt = (prev + 1) % M
    return w, prev, nxt, frac


def forward(x, mod, consts, M, book=None, frac64=None):
    """fp64 forward from the fp32 slots (frac64 overrides the fractions, for finite differences).  Returns a dict with
    y, z, o, the tap v and the two values read, d_prev / d_next (all (B, N) fp64), and z32, the fp32 forward's z."""
    x = np.asarray(x)
    B, N = x.shape
    w, prev, nxt, frac = book if book is not None else bookkeeping(mod, consts, M)
    f64 = frac.astype(np.float64) if frac64 is None else frac64
    c = {k: np.asarray(v, np.float64) for k, v in consts.items()}
    c32 = {k: np.asarray(v, F32) for k, v in consts.items()}
    x64, x32 = x.astype(np.float64), x.astype(F32)
    omf32 = (F32(1.0) - frac).astype(F32)
    bi = np.arange(B)
    ring, ring32 = np.zeros((B, M)), np.zeros((B, M), F32)
    v, dp_, dn_ = np.empty((B, N)), np.empty((B, N)), np.empty((B, N))
    v32 = np.empty((B, N), F32)
    for n in range(N):
        p, q = prev[:, n], nxt[:, n]
        a, b = ring[bi, p], ring[bi, q]
        dp_[:, n], dn_[:, n] = a, b
        t = f64[:, n] * b + (1.0 - f64[:, n]) * a
        v[:, n] = t
        ring[:, w[n]] = x64[:, n] + c["feedback"] * t
        t32 = ((frac[:, n] * ring32[bi, q]).astype(F32) + (omf32[:, n] * ring32[bi, p]).astype(F32)).astype(F32)
        v32[:, n] = t32
        ring32[:, w[n]] = (x32[:, n] + (c32["feedback"] * t32).astype(F32)).astype(F32)
    o = x64 + c["depth"][:, None] * v
    z = c["one_minus_mix"][:, None] * x64 + c["mix"][:, None] * o
    o32 = (x32 + (c32["depth"][:, None] * v32).astype(F32)).astype(F32)
    z32 = ((c32["one_minus_mix"][:, None] * x32).astype(F32) + (c32["mix"][:, None] * o32).astype(F32)).astype(F32)
    return {"y": np.clip(z, -1.0, 1.0), "z": z, "o": o, "v": v, "d_prev": dp_, "d_next": dn_, "z32": z32,
            "y32": np.clip(z32, F32(-1.0), F32(1.0)), "v32": v32}


def flanger_adjoint64(x, mod, consts, M, dy, fwd=None):
    """Gradients of sum(dy * y): dx, dmod (B, N) and the per-clip lfo_scale, min_delay, feedback, depth, mix (B,) (mix
    through both mix and one_minus_mix = 1 - mix), all fp64.  Also returns the forward dict under "fwd"."""
    x = np.asarray(x)
    B, N = x.shape
    book = bookkeeping(mod, consts, M)
    w, prev, nxt, frac = book
    fwd = fwd if fwd is not None else forward(x, mod, consts, M, book)
    c = {k: np.asarray(v, np.float64) for k, v in consts.items()}
    f64 = frac.astype(np.float64)
    x64, dy64 = x.astype(np.float64), np.asarray(dy, np.float64)
    z32 = fwd["z32"]
    gz = np.where((z32 >= -1.0) & (z32 <= 1.0), dy64, 0.0)
    go = c["mix"][:, None] * gz
    bi = np.arange(B)
    A = np.zeros((B, M))
    gd = np.empty((B, N))
    dpth, fb = c["depth"], c["feedback"]
    for n in range(N - 1, -1, -1):                  # reverse of (read prev / next, then write w)
        gd[:, n] = A[:, w[n]]
        A[:, w[n]] = 0.0
        gv = dpth * go[:, n] + fb * gd[:, n]
        A[bi, prev[:, n]] += (1.0 - f64[:, n]) * gv
        A[bi, nxt[:, n]] += f64[:, n] * gv
    gv = dpth[:, None] * go + fb[:, None] * gd
    gf = gv * (fwd["d_next"] - fwd["d_prev"])
    mod64 = np.asarray(mod, np.float64)
    return {"dx": c["one_minus_mix"][:, None] * gz + go + gd,
            "dmod": -c["lfo_scale"][:, None] * gf,
            "lfo_scale": -(gf * mod64).sum(1),
            "min_delay": -gf.sum(1),
            "feedback": (gd * fwd["v"]).sum(1),
            "depth": (go * fwd["v"]).sum(1),
            "mix": (gz * (fwd["o"] - x64)).sum(1),
            "g_d": gd, "fwd": fwd}

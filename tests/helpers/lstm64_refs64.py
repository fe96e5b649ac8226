"""Independent fp64 references of the LSTM-64 effect model (reference models.py:311-339: nn.LSTM(2, 64) on (lfo, audio) ->
Linear(64, 1) -> + x -> tanh) and of its truncated BPTT, with a per-element error bound computed beside every value from sums
of magnitudes -- the yardstick of the kernels of csrc/lstm.hip (mx_lstm_fwd, mx_lstm_bwd_l1, mx_lstm_bwd, mx_lstm_bwd_dgate,
mx_lstm_dlfo) in tests/test_gpu_lstm64_units.py.  numpy only; the forward recurrence is general_refs64.lstmg_fwd, which shares
nothing with lstm.hip.  tests/test_lstm64_refs64.py holds the references to torch autograd in fp64, a plain fp32 emulation of
the same formulae (``emu_fwd`` / ``emu_bwd``) to every bound, and that emulation with one seeded defect at a time to the gates.

u = 2^-23, gamma(n) = n u / (1 - n u).  Outside the activation model every fp32 operation is charged u of the magnitude of its
result (twice round-to-nearest's u / 2: the convention of gamma); products of two error terms are kept where they are formed.

Activation model (``act_bound``).  The kernel evaluates A_s(x) = s sigmoid(s x) + 1 - s (s = 1: sigmoid, s = 2: tanh) as
    a = fl(x * c_s),  c_s = fl32(-s log2 e)      e = v_exp_f32(a)      d = fl(1 + e)      r = v_rcp_f32(d)      fma(r, s, 1 - s)
and the header of lstm.hip documents v_exp_f32 and v_rcp_f32 at 1 ulp (<= u relative) each.
  * argument: c_s carries <= u / 2 relative, the product another u / 2, so a = s x log2(e) (1 + d), |d| <= u, and
    2^a = e (1 + eta_a) with |eta_a| = ln 2 |a| u = s |x| u; with the instruction's own ulp: e^ = e (1 + eta), |eta| <= (s |x| + 1) u;
  * sigma = 1 / (1 + e) has d sigma / d e = -sigma^2, so eta moves it by sigma^2 e eta = sigma (1 - sigma) eta;
  * d rounds by u / 2 and r by u, both relative to sigma: 1.5 u sigma;
  * s = 1: fma(r, 1, 0) = r exactly.      |sigmoid^ - sigmoid| <= sigma (1 - sigma) (|x| + 1) u + 1.5 u sigma
  * s = 2: 2 r - 1 is rounded once: u / 2 of |tanh|, and the two terms above double (sigma taken at 2 x):
                                          |tanh^ - tanh| <= 2 [sigma (1 - sigma) (2 |x| + 1) u + 1.5 u sigma] + (u / 2) |tanh x|
Second-order terms are covered by a factor 1 + 2^-10, a flushed e (below 2^-126, x > 87) by 2^-126 absolute.  Nothing here is
fitted to device output.

tanhf (the output layer's): the ROCm installation ships the device library as bitcode only and states no accuracy for it, so
the OpenCL full-profile figure is used: 5 ulp.
"""
import functools

import numpy as np

from tests.helpers import general_refs64 as G

f32, f64 = np.float32, np.float64
U = 2.0 ** -23
H, NG, STASH, NPARAM = 64, 256, 384, 17473
TANHF_ULP = 5.0
SLACK = 1.0 + 2.0 ** -10
gamma = G.gamma
LOG2E32 = f32(1.4426950408889634)
D2_SIG, D2_TANH = 0.0963, 0.7699                   # sup |sigmoid''|, sup |tanh''|
# state-dict order of one ``part`` row
PARTS = {"w_ih": (0, 512), "w_hh": (512, 16896), "b_ih": (16896, 17152), "b_hh": (17152, 17408), "fc_w": (17408, 17472),
         "fc_b": (17472, 17473)}


def ratio(got, ref, bound):
    """Worst |got - ref| / bound (0 where the difference is 0: a zero bound demands equality); inf if ``got`` has a NaN."""
    got = np.asarray(got, f64)
    if np.isnan(got).any():
        return float("inf")
    err = np.abs(got - np.asarray(ref, f64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / np.maximum(np.asarray(bound, f64), 1e-300))
    return float(np.max(r)) if r.size else 0.0


# ---- activations ----------------------------------------------------------------------------------------------------------
def act_bound(x, s):
    """Absolute error bound of the kernel's sigmoid (s = 1) / tanh (s = 2) at the fp32 argument x (derivation: module docstring)."""
    x = np.asarray(x, f64)
    assert np.all(np.abs(s * x) < 80.0), "outside the range the activation model was derived for (e overflows / is flushed)"
    sg = G.sigmoid(s * x)
    b = sg * (1.0 - sg) * (s * np.abs(x) + 1.0) * U + 1.5 * U * sg
    if s == 2:
        b = 2.0 * b + 0.5 * U * np.abs(2.0 * sg - 1.0)
    return b * SLACK + 2.0 ** -126


def _gate(pre, e_pre, s):
    """Value, bound of the activation of a pre-activation known to e_pre: |act'| e_pre + sup|act''| e_pre^2 / 2 + act_bound."""
    if s == 1:
        a = G.sigmoid(pre)
        d1, d2 = a * (1.0 - a), D2_SIG
    else:
        a = np.tanh(pre)
        d1, d2 = 1.0 - a * a, D2_TANH
    return a, d1 * e_pre + 0.5 * d2 * e_pre * e_pre + act_bound(pre, s)


def _w(p, *names):
    return [np.asarray(p[n], f64) for n in names]


# ---- forward ----------------------------------------------------------------------------------------------------------------
def step_fwd(p, lfo, x, h_prev, c_prev):
    """One step from the state AS THE DEVICE LEFT IT: lfo, x (...), h_prev, c_prev (..., 64) -> ({i, f, g, o, c, h}, bounds).
    Pre-activations: gamma(64 + 4) of the magnitudes of the 66 products and two biases; gates: _gate; c = fma(f, c_prev, i g)
    and h = o tanh(c): the product rule plus u per fp32 operation.  Nothing accumulates across steps."""
    w_ih, w_hh, b_ih, b_hh = _w(p, "w_ih", "w_hh", "b_ih", "b_hh")
    lfo, x = np.asarray(lfo, f64)[..., None], np.asarray(x, f64)[..., None]
    h_prev, c_prev = np.asarray(h_prev, f64), np.asarray(c_prev, f64)
    pre = lfo * w_ih[:, 0] + x * w_ih[:, 1] + b_ih + b_hh + h_prev @ w_hh.T
    mag = np.abs(lfo * w_ih[:, 0]) + np.abs(x * w_ih[:, 1]) + np.abs(b_ih) + np.abs(b_hh) + np.abs(h_prev) @ np.abs(w_hh).T
    e_pre = gamma(H + 4) * mag
    v, e = {}, {}
    for q, name in enumerate("ifgo"):
        v[name], e[name] = _gate(pre[..., q * H:(q + 1) * H], e_pre[..., q * H:(q + 1) * H], 2 if name == "g" else 1)
    fc, ig = v["f"] * c_prev, v["i"] * v["g"]
    v["c"] = fc + ig
    e["c"] = (e["f"] * np.abs(c_prev) + e["i"] * np.abs(v["g"]) + e["g"] * np.abs(v["i"]) + e["i"] * e["g"]
              + U * (np.abs(fc) + np.abs(ig))) * SLACK
    tc = np.tanh(v["c"])
    e_tc = (1.0 - tc * tc) * e["c"] + 0.5 * D2_TANH * e["c"] ** 2 + act_bound(v["c"], 2)
    v["h"] = v["o"] * tc
    e["h"] = (e["o"] * np.abs(tc) + np.abs(v["o"]) * e_tc + e["o"] * e_tc + U * np.abs(v["h"])) * SLACK
    return v, e


def y_fwd(p, h, x):
    """y_t = tanhf(fc_b + sum_k fc_w[k] h_t[k] + x_t) from the DEVICE's h_t (..., 64): a 64-term fma chain and one addition
    (gamma(64 + 2) of the magnitudes) through tanh's slope, plus tanhf's TANHF_ULP ulp of |y|."""
    fc_w, fc_b = _w(p, "fc_w", "fc_b")
    h, x = np.asarray(h, f64), np.asarray(x, f64)
    pre = fc_b[0] + h @ fc_w + x
    e_pre = gamma(H + 2) * (abs(fc_b[0]) + np.abs(h) @ np.abs(fc_w) + np.abs(x))
    y = np.tanh(pre)
    return y, ((1.0 - y * y) * e_pre + 0.5 * D2_TANH * e_pre ** 2 + TANHF_ULP * U * np.abs(y)) * SLACK


def fwd64(p):
    """The whole chunk in fp64: stash (B, T, 384) = (i, f, g, o, c, h) of every step, y (B, T), h_out, c_out (B, 64)."""
    w_ih, w_hh, b_ih, b_hh, fc_w, fc_b = _w(p, "w_ih", "w_hh", "b_ih", "b_hh", "fc_w", "fc_b")
    lfo, x = np.asarray(p["lfo"], f64), np.asarray(p["x"], f64)
    zin = lfo[..., None] * w_ih[:, 0] + x[..., None] * w_ih[:, 1]
    st, h1, c1 = G.lstmg_fwd(zin, b_ih, b_hh, w_hh, p["h_in"], p["c_in"])
    B, T = x.shape
    return st.reshape(B, T, STASH), np.tanh(st[:, :, 5] @ fc_w + fc_b[0] + x), h1, c1


def fwd_gates(p, stash, y, h_out, c_out):
    """The comparisons of the forward GPU test on a run's outputs: every stash row against step_fwd of the previous row of the
    SAME run (h_in / c_in for row 0), y against y_fwd of the run's own h, h_out / c_out bit-equal to the last row's planes.
    Returns {gate: worst ratio} (``state``: 0 or inf)."""
    st = np.asarray(stash, f32)
    B, T = st.shape[:2]
    h_prev = np.concatenate([np.asarray(p["h_in"], f32)[:, None], st[:, :-1, 320:]], 1)
    c_prev = np.concatenate([np.asarray(p["c_in"], f32)[:, None], st[:, :-1, 256:320]], 1)
    if np.isnan(h_prev).any() or np.isnan(c_prev).any() or np.isnan(st).any():
        return {k: float("inf") for k in "ifgochy"} | {"state": float("inf")}
    v, e = step_fwd(p, p["lfo"], p["x"], h_prev, c_prev)
    out = {name: ratio(st[:, :, q * H:(q + 1) * H], v[name], e[name]) for q, name in enumerate("ifgoch")}
    yr, ye = y_fwd(p, st[:, :, 320:], p["x"])
    out["y"] = ratio(y, yr, ye)
    same = (np.array_equal(np.asarray(h_out, f32).view(np.int32), np.ascontiguousarray(st[:, -1, 320:]).view(np.int32))
            and np.array_equal(np.asarray(c_out, f32).view(np.int32), np.ascontiguousarray(st[:, -1, 256:320]).view(np.int32)))
    out["state"] = 0.0 if same else float("inf")
    return out


# ---- backward ---------------------------------------------------------------------------------------------------------------
def loss_grad(p, y, mode):
    """d loss / d y (B, T): ``l1`` = loss_scale sign(y - wet) with sign(0) = 0 (nn.L1Loss), ``dy`` = the problem's random dy."""
    if mode == "dy":
        return np.asarray(p["dy"], f64)
    return float(p["loss_scale"]) * np.sign(np.asarray(y, f64) - np.asarray(p["wet"], f64))


def _bptt(p, stash, y, g, dgate_dev=None):
    """The BPTT of one chunk in fp64 for a GIVEN stash (B, T, 384), y and g = d loss / d y, with the error recurrence of the
    kernel's arithmetic beside it.  dgate_dev None: the running bound (bwd_running).  dgate_dev (B, T, 256), the device's own
    gate gradients: step t takes dh_t from dgate_dev[t + 1] (step_bwd), which carries no inherited error.
    Per step (u per fp32 operation):
      dzy = g (1 - y^2): y^2, the subtraction and the product round: <= u |g|                  (y^2 + 2 (1 - y^2) <= 2)
      dh  = fc_w dzy + W_hh^T dg(t+1): gamma(256 + 2) of the magnitudes (+ |W_hh|^T E_dg(t+1) when running)
      tc  = the kernel's tanh of the stashed c: act_bound;  kc = o (1 - tc^2);  dc = fma(dh, kc, dc');  dc' = dc f
      dg  = (dh | dc) * der * partner, der = a (1 - a) | 1 - a^2 (two roundings: u |der|)
    s_dgate is the magnitude sum of every element, the scale the sharpness condition of bwd_running is relative to: the terms
    that are ADDED to form it -- |W_hh|^T |dg(t+1)| + |fc_w dzy| for dh; that times |kc| plus the magnitude sum carried with
    dc' (a chain with the factor f < 1 only) for dc -- times the local factor.  One exception: the kernel forms tanh(c) as
    2 sigmoid(2 c) - 1, a cancellation at c ~ 0 whose absolute error is ~2 u whatever |tanh c| is, so the o gate's factor
    |tanh c| is replaced by the magnitude sum of that subtraction, 2 sigmoid(2 c) + 1."""
    w_hh, fc_w = _w(p, "w_hh", "fc_w")
    aW = np.abs(w_hh)
    st = np.asarray(stash, f64)
    B, T = st.shape[:2]
    st = st.reshape(B, T, 6, H)
    y, g = np.asarray(y, f64), np.asarray(g, f64)
    dzy, e_dzy = g * (1.0 - y * y), U * np.abs(g)
    running = dgate_dev is None
    dgd = None if running else np.asarray(dgate_dev, f64)
    dgate, e_dgate, s_dgate = (np.zeros((B, T, NG)) for _ in range(3))
    dg_n = e_n = np.zeros((B, NG))
    dcn = e_dcn = m_dcn = np.zeros((B, H))
    c_in = np.asarray(p["c_in"], f64)
    for t in range(T - 1, -1, -1):
        i, f, gg, o, c = (st[:, t, q] for q in range(5))
        cp = st[:, t - 1, 4] if t > 0 else c_in
        if running or t == T - 1:
            src, e_src = dg_n, e_n
        else:
            src, e_src = dgd[:, t + 1], None
        zf = dzy[:, t, None] * fc_w
        dh = zf + src @ w_hh
        mag = np.abs(src) @ aW + np.abs(zf)
        e_dh = gamma(NG + 2) * mag + e_dzy[:, t, None] * np.abs(fc_w)
        if running:
            e_dh = e_dh + e_src @ aW
        tc, e_tc = np.tanh(c), act_bound(c, 2)
        kc = o * (1.0 - tc * tc)
        e_kc = np.abs(o) * (2.0 * np.abs(tc) * e_tc + e_tc * e_tc) + U * np.abs(kc)
        dc = dh * kc + dcn
        e_dc = e_dh * np.abs(kc) + np.abs(dh) * e_kc + e_dh * e_kc + e_dcn + U * (np.abs(dh * kc) + np.abs(dcn))
        m_dc = mag * np.abs(kc) + m_dcn
        dcn, e_dcn, m_dcn = dc * f, e_dc * np.abs(f) + U * np.abs(dc * f), m_dc * np.abs(f)
        for q, (a, prt, e_prt) in enumerate(((i, gg, 0.0), (f, cp, 0.0), (gg, i, 0.0), (o, tc, e_tc))):
            der = 1.0 - a * a if q == 2 else a * (1.0 - a)
            kq = der * prt
            e_kq = U * np.abs(der) * (np.abs(prt) + e_prt) + np.abs(der) * e_prt + U * np.abs(kq)
            s_, e_s, m_s = (dh, e_dh, mag) if q == 3 else (dc, e_dc, m_dc)
            sl = slice(q * H, (q + 1) * H)
            dgate[:, t, sl] = s_ * kq
            e_dgate[:, t, sl] = e_s * np.abs(kq) + np.abs(s_) * e_kq + e_s * e_kq + U * np.abs(s_ * kq)
            s_dgate[:, t, sl] = m_s * np.abs(der) * (2.0 * G.sigmoid(2.0 * c) + 1.0) if q == 3 else m_s * np.abs(kq)
        dg_n, e_n = dgate[:, t], e_dgate[:, t]
    return dict(dgate=dgate, e_dgate=e_dgate, s_dgate=s_dgate, dzy=dzy, e_dzy=e_dzy)


def _part(p, stash, dgate, e_dgate, s_dgate, dzy, e_dzy):
    """part (B, 17473), state-dict order, as fp64 sums over t of dgate_t (x) (lfo_t, x_t), dgate_t (x) h_{t-1}, dgate_t (both
    bias rows), dzy_t h_t, dzy_t.  Bound: sum_t E_dg_t |h_{t-1}| + gamma(T + 4) sum_t |dg_t| |h_{t-1}| (and alike); the third
    value is the magnitude sum the bound is relative to (from s_dgate)."""
    st = np.asarray(stash, f64)
    B, T = st.shape[:2]
    h = st[:, :, 320:]
    h_prev = np.concatenate([np.asarray(p["h_in"], f64)[:, None], h[:, :-1]], 1)
    inp = np.stack([np.asarray(p["lfo"], f64), np.asarray(p["x"], f64)], -1)           # (B, T, 2)
    one = np.ones((B, T, 1))
    gT = gamma(T + 4)
    val, bnd, mag = (np.zeros((B, NPARAM)) for _ in range(3))

    def put(name, d, e_d, m_d, other):
        lo, hi = PARTS[name]
        ao = np.abs(other)
        val[:, lo:hi] = np.einsum("btr,btk->brk", d, other).reshape(B, -1)
        sm = np.einsum("btr,btk->brk", np.abs(d), ao).reshape(B, -1)
        bnd[:, lo:hi] = np.einsum("btr,btk->brk", e_d, ao).reshape(B, -1) + gT * sm
        mag[:, lo:hi] = np.einsum("btr,btk->brk", m_d, ao).reshape(B, -1)
    put("w_ih", dgate, e_dgate, s_dgate, inp)
    put("w_hh", dgate, e_dgate, s_dgate, h_prev)
    put("b_ih", dgate, e_dgate, s_dgate, one)
    put("b_hh", dgate, e_dgate, s_dgate, one)
    z, ez = dzy[..., None], e_dzy[..., None]
    put("fc_w", z, ez, np.abs(z), h)
    put("fc_b", z, ez, np.abs(z), one)
    return val, bnd, mag


def bwd_running(p, stash, y, g, sharp=2.0 ** -10):
    """Full fp64 BPTT with the running bound: dict(dgate, e_dgate, part, e_part).  Asserts that every bound is at most
    ``sharp`` of its element's magnitude sum: the condition that keeps the gate sharp (it holds for contractive weights)."""
    r = _bptt(p, stash, y, g)
    part, e_part, m_part = _part(p, stash, r["dgate"], r["e_dgate"], r["s_dgate"], r["dzy"], r["e_dzy"])
    assert np.all(r["e_dgate"] <= sharp * r["s_dgate"]), float(np.max(r["e_dgate"] / np.maximum(r["s_dgate"], 1e-300)))
    assert np.all(e_part <= sharp * m_part), float(np.max(e_part / np.maximum(m_part, 1e-300)))
    r.update(part=part, e_part=e_part)
    return r


def step_bwd(p, stash, y, g, dgate_dev):
    """dgate[t] from the DEVICE's dgate[t + 1] (local bound; dc is carried by the reference: its error recurrence has only the
    factor f < 1): dict(dgate, e_dgate)."""
    return _bptt(p, stash, y, g, dgate_dev)


def part_from_dgate(p, stash, y, g, dgate_dev):
    """part from the DEVICE's dgate: (value, bound)."""
    y, g = np.asarray(y, f64), np.asarray(g, f64)
    d = np.asarray(dgate_dev, f64)
    val, bnd, _ = _part(p, stash, d, np.zeros_like(d), np.abs(d), g * (1.0 - y * y), U * np.abs(g))
    return val, bnd


def part_ratios(part, ref, bound):
    """{parameter tensor: worst ratio} of part (B, 17473), and ``bias`` = 0 if the two bias rows are bit-equal (else inf)."""
    part = np.asarray(part, f32)
    out = {n: ratio(part[:, lo:hi], ref[:, lo:hi], bound[:, lo:hi]) for n, (lo, hi) in PARTS.items()}
    bi, bh = (np.ascontiguousarray(part[:, slice(*PARTS[n])]).view(np.int32) for n in ("b_ih", "b_hh"))
    out["bias"] = 0.0 if np.array_equal(bi, bh) else float("inf")
    return out


def dlfo64(p, dgate):
    """dlfo[b][t] = sum_r w_ih[r][0] dgate[b][t][r] and gamma(256 + 2) of the magnitudes."""
    w0, d = np.asarray(p["w_ih"], f64)[:, 0], np.asarray(dgate, f64)
    return d @ w0, gamma(NG + 2) * (np.abs(d) @ np.abs(w0))


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def problem(kind, B, T):
    """Read-only inputs.  ``default``: every weight uniform in +-1/8 (nn.LSTM's own range); ``hot``: the default set with w_ih
    and both biases x 8 (gates saturate: the |x| term of act_bound matters); ``contractive``: w_hh in +-1/32 (the running
    bound of the BPTT stays within 2^-10 of the magnitude sums at every T).  x in +-0.8, lfo in [0, 1], non-zero h_in / c_in,
    wet = y + noise with a quarter of the samples, the first and the last EXACTLY equal to y; a random dy.  ``stash`` / ``y``: the fp64 forward rounded to fp32,
    independent of the forward kernel -- the backward tests' input."""
    g = np.random.default_rng([{"default": 1, "hot": 2, "contractive": 3}[kind], B, T])
    un = lambda a, shape: g.uniform(-a, a, shape).astype(f32)
    p = dict(kind=kind, B=B, T=T, w_ih=un(0.125, (NG, 2)), w_hh=un(1 / 32 if kind == "contractive" else 0.125, (NG, H)),
             b_ih=un(0.125, NG), b_hh=un(0.125, NG), fc_w=un(0.125, H), fc_b=un(0.125, 1), x=un(0.8, (B, T)),
             lfo=g.uniform(0.0, 1.0, (B, T)).astype(f32), h_in=un(0.5, (B, H)), c_in=un(1.0, (B, H)), dy=un(1.0, (B, T)))
    if kind == "hot":
        for n in ("w_ih", "b_ih", "b_hh"):
            p[n] = p[n] * f32(8)
    p["loss_scale"] = float(f32(1.0 / (B * T)))
    st, y, h1, c1 = fwd64(p)
    p.update(stash=st.astype(f32), y=y.astype(f32), h_out64=h1, c_out64=c1, stash64=st, y64=y)
    wet = (y + g.normal(0.0, 0.05, (B, T))).astype(f32)
    ties = g.random((B, T)) < 0.25
    ties[:, 0] = ties[:, -1] = True
    wet[ties] = p["y"][ties]
    p["wet"], p["ties"] = wet, ties
    for v in p.values():
        if isinstance(v, np.ndarray):
            _ro(v)
    return p


@functools.lru_cache(maxsize=None)
def running_ref(kind, B, T, mode):
    """bwd_running of problem(kind, B, T) on its own stash / y, ``mode`` l1 | dy; arrays read-only."""
    p = problem(kind, B, T)
    r = bwd_running(p, p["stash"], p["y"], loss_grad(p, p["y"], mode))
    return {k: _ro(v) for k, v in r.items()}


# ---- plain fp32 emulation of the same formulae (sequential sums, exp2 / reciprocal perturbed by +-1 ulp) --------------------
def _perturb(v, rng):
    if rng is None:
        return v
    k = rng.integers(-1, 2, v.shape)
    return np.where(k == 0, v, np.nextafter(v, np.where(k > 0, f32(np.inf), f32(-np.inf)).astype(f32))).astype(f32)


def _act32(x, s, rng, rel=0.0):
    x = np.asarray(x, f32)
    e = _perturb(np.exp2((x * (f32(-s) * LOG2E32)).astype(f64)).astype(f32), rng)
    r = _perturb((1.0 / (f32(1) + e).astype(f64)).astype(f32), rng)
    a = r * f32(s) + f32(1 - s)
    return (a * f32(1.0 + rel)).astype(f32) if rel else a


def _seqdot(a, b):
    """sum over the last axis of a * b, products rounded, accumulated sequentially in fp32."""
    return np.add.accumulate((np.asarray(a, f32) * np.asarray(b, f32)), axis=-1, dtype=f32)[..., -1]


FWD_DEFECTS = ("stash_early", "swap_in", "no_bhh", "c_restart", "act_err")
BWD_DEFECTS = ("drop_dg1_h0", "dg0_h0", "skip_last_slab", "f_carry", "tanh_prev_row", "no_bias_hh", "sign0", "df0_zero_cinit")


def emu_fwd(p, rng=None, defect=None):
    """fp32 forward; the outputs start as NaN (the sentinel of the GPU tests).  Returns (stash (B, T, 384), y, h_out, c_out).
    ``defect``: one of FWD_DEFECTS --
      stash_early: the stash row of a 256-step block's last step lands one row early;   swap_in: lfo and x swapped;
      no_bhh: b_hh dropped;   c_restart: c of the second 256-step block restarts from c_in;   act_err: every activation is
      2^-18 relatively off."""
    assert defect is None or defect in FWD_DEFECTS
    w_ih, w_hh, b_ih, b_hh, fc_w = (np.asarray(p[n], f32) for n in ("w_ih", "w_hh", "b_ih", "b_hh", "fc_w"))
    x, lfo = np.asarray(p["x"], f32), np.asarray(p["lfo"], f32)
    B, T = x.shape
    if defect == "swap_in":
        x_in, lfo_in = lfo, x
    else:
        x_in, lfo_in = x, lfo
    bias = b_ih if defect == "no_bhh" else b_ih + b_hh
    rel = 2.0 ** -18 if defect == "act_err" else 0.0
    h, c = np.asarray(p["h_in"], f32).copy(), np.asarray(p["c_in"], f32).copy()
    stash = np.full((B, T, STASH), np.nan, f32)
    hs = np.zeros((B, T, H), f32)                                  # the LDS history: y is formed from it, not from the stash
    for t in range(T):
        if defect == "c_restart" and t == 256:
            c = np.asarray(p["c_in"], f32).copy()
        acc = w_ih[:, 0] * lfo_in[:, t, None] + bias
        acc = w_ih[:, 1] * x_in[:, t, None] + acc
        for k in range(H):
            acc = acc + w_hh[:, k] * h[:, k, None]
        gi, gf, go = (_act32(acc[:, q * H:(q + 1) * H], 1, rng, rel) for q in (0, 1, 3))
        gg = _act32(acc[:, 2 * H:3 * H], 2, rng, rel)
        c = gf * c + gi * gg
        h = go * _act32(c, 2, rng, rel)
        row = t
        if defect == "stash_early" and (t % 256 == 255 or t == T - 1) and t > 0:
            row = t - 1
        stash[:, row] = np.concatenate([gi, gf, gg, go, c, h], -1)
        hs[:, t] = h
    acc = np.broadcast_to(np.asarray(p["fc_b"], f32)[0], (B, T)).astype(f32)
    for k in range(H):
        acc = acc + fc_w[k] * hs[:, :, k]
    y = np.tanh((acc + x).astype(f64)).astype(f32)
    return stash, y, h.copy(), c.copy()


def emu_bwd(p, stash, y, mode, rng=None, defect=None):
    """fp32 BPTT of the given stash / y; ``mode`` l1 | dy.  Returns (dgate (B, T, 256), part (B, 17473)), NaN where never
    written.  ``defect``: one of BWD_DEFECTS --
      drop_dg1_h0: step 1's products left out of the weight / bias sums (the odd-T left-over pair);
      dg0_h0: dg(0) multiplied with h_0 instead of h_in;   skip_last_slab: the last step skipped when T = 1 mod 32, T > 32;
      f_carry: the dc carry into step t uses f_t instead of f_{t+1};   tanh_prev_row: tanh(c) from row t - 1;
      no_bias_hh: the bias_hh row not written;   sign0: sign(0) = 1;   df0_zero_cinit: df at t = 0 from a zero c_in."""
    assert defect is None or defect in BWD_DEFECTS
    w_hh, fc_w = np.asarray(p["w_hh"], f32), np.asarray(p["fc_w"], f32)
    st = np.asarray(stash, f32)
    B, T = st.shape[:2]
    st = st.reshape(B, T, 6, H)
    y = np.asarray(y, f32)
    if mode == "dy":
        g = np.asarray(p["dy"], f32)
    else:
        e = y - np.asarray(p["wet"], f32)
        sg = np.sign(e)
        if defect == "sign0":
            sg = np.where(e == 0, f32(1), sg)
        g = (f32(p["loss_scale"]) * sg).astype(f32)
    dzy = g * (f32(1) - y * y)
    x, lfo = np.asarray(p["x"], f32), np.asarray(p["lfo"], f32)
    h_in, c_in = np.asarray(p["h_in"], f32), np.asarray(p["c_in"], f32)
    dgate = np.full((B, T, NG), np.nan, f32)
    part = np.full((B, NPARAM), np.nan, f32)
    a_ih, a_hh, a_b = np.zeros((B, NG, 2), f32), np.zeros((B, NG, H), f32), np.zeros((B, NG), f32)
    a_fw, a_fb = np.zeros((B, H), f32), np.zeros(B, f32)
    dg = np.zeros((B, NG), f32)
    dc_prev, f_next = np.zeros((B, H), f32), np.zeros((B, H), f32)
    one = f32(1)
    for t in range(T - 1, -1, -1):
        i, f, gg, o, c, h = (st[:, t, q] for q in range(6))
        if defect == "skip_last_slab" and t == T - 1 and T % 32 == 1 and T > 32:
            dgate[:, t] = 0
            continue
        cp = st[:, t - 1, 4] if t > 0 else (np.zeros_like(c_in) if defect == "df0_zero_cinit" else c_in)
        dhn = _seqdot(w_hh.T[None], dg[:, None, :])
        dh = dzy[:, t, None] * fc_w + dhn
        tc = _act32(st[:, t - 1, 4] if defect == "tanh_prev_row" and t > 0 else c, 2, rng)
        kc = o * (one - tc * tc)
        dcn = dc_prev * (f if defect == "f_carry" else f_next)
        dc = dh * kc + dcn
        dc_prev, f_next = dc, f
        dg = np.concatenate([dc * ((i * (one - i)) * gg), dc * ((f * (one - f)) * cp), dc * ((one - gg * gg) * i),
                             dh * ((o * (one - o)) * tc)], -1).astype(f32)
        dgate[:, t] = dg
        a_fw = a_fw + dzy[:, t, None] * h
        a_fb = a_fb + dzy[:, t]
        if defect == "drop_dg1_h0" and t == 1 and T % 2 == 1:
            continue
        hp = st[:, t - 1, 5] if t > 0 else (st[:, 0, 5] if defect == "dg0_h0" else h_in)
        a_hh = a_hh + dg[:, :, None] * hp[:, None, :]
        a_ih = a_ih + dg[:, :, None] * np.stack([lfo[:, t], x[:, t]], -1)[:, None, :]
        a_b = a_b + dg
    for n, a in (("w_ih", a_ih), ("w_hh", a_hh), ("b_ih", a_b), ("b_hh", a_b), ("fc_w", a_fw), ("fc_b", a_fb)):
        if n == "b_hh" and defect == "no_bias_hh":
            continue
        part[:, slice(*PARTS[n])] = a.reshape(B, -1)
    return dgate, part

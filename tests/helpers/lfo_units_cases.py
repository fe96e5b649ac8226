"""The inputs of tests/test_gpu_lfo_units.py, shared with tests/test_lfo_units64.py (which checks the exclusion caps and the
helpers on exactly these sizes), and the oracle's own fp32 error against the fp64 references of tests/helpers/lfo_units64.py --
the figure every derived gate of the GPU file is a multiple of.  Nothing here touches a device."""
import functools
import math

import numpy as np

from tests.helpers import lfo_units64 as L

f32, f64 = np.float32, np.float64

# ==== mx_lfo_synth =============================================================================================================
RATES = (0.1, 0.5, 2.7, 7.9)
SRS = (441.0, 172.5, 44100.0)
STARTS = (0, 1, 44099, 2 ** 20)
EXPS = (1.0, 2.0, 3.0, 0.5, 1.7)
N_SRC = (1, 255, 256, 257, 882)
SYNTH_B = 7
MARGIN_SYNTH, CAP_SYNTH = 1e-5, 0.01


@functools.lru_cache(None)
def synth_cases():
    """One launch each: 7 rows, one per shape (all cos where the shape pointer is null).  Every (n_src, n_out) pair runs five
    variants: start null / exp null / (at n_src = 255) shape null / two with all three given; rates, sample rates, starts and
    exponents rotate through their sets so that every shape meets every exponent."""
    cases, c = [], 0
    for n_src in N_SRC:
        for n_out in dict.fromkeys((n_src, 1, 345, 2 * n_src + 1)):
            if n_src == 1 and n_out > 1:
                continue                                   # the reference's interpolation needs two points to stretch
            for v in range(5):
                b = np.arange(SYNTH_B)
                cases.append(dict(
                    name=f"{n_src}to{n_out}_v{v}", n_src=n_src, n_out=n_out, sr=SRS[(c + v) % 3],
                    freq=np.array([RATES[(i + c) % 4] for i in b], f32),
                    phase=(-6.0 + 1.9 * ((b + v) % 7)).astype(f32),
                    shape=None if (v == 2 and n_src == 255) else b.astype(np.int32),
                    exp=None if v == 1 else np.array([EXPS[(i + v + c) % 5] for i in b], f32),
                    start=None if v == 0 else np.array([STARTS[(i + c + v) % 4] for i in b], np.int32)))
            c += 1
    return cases


def synth_ref(case):
    return L.lfo_synth64(case["freq"], case["phase"], case["shape"], case["exp"], case["start"], case["n_src"], case["n_out"],
                         case["sr"])


def synth_row_params(case, b):
    sh = L.COS if case["shape"] is None else int(case["shape"][b])
    e = 1.0 if case["exp"] is None else float(case["exp"][b])
    st = 0 if case["start"] is None else int(case["start"][b])
    return sh, e, st


def oracle_signal(n, sr, freq, phase, shape, exp, start=0):
    """oracle.modulations.make_mod_signal for the points start .. start + n - 1 of a longer signal: its own code with its own
    closed-form phase evaluated at k + start (tests/test_lfo_units64.py holds this against cropping the long signal)."""
    from oracle import modulations as omod
    own = omod.lfo_argument

    def shifted(n_samples, sr_, f_, ph_):
        k = np.arange(1 + start, n_samples + 1 + start, dtype=np.float64)
        return ((k * np.float64(omod.lfo_step(sr_, f_))).astype(f32) + f32(ph_)).astype(f32)

    omod.lfo_argument = shifted
    try:
        return omod.make_mod_signal(n, sr, float(freq), float(phase), L.SHAPES[shape], float(exp)).numpy()
    finally:
        omod.lfo_argument = own


def oracle_synth(case):
    from oracle import util as outil
    rows = []
    for b in range(SYNTH_B):
        sh, e, st = synth_row_params(case, b)
        rows.append(oracle_signal(case["n_src"], case["sr"], case["freq"][b], case["phase"][b], sh, f32(e), st))
    return outil.linear_interpolate_last_dim_np(np.stack(rows), case["n_out"])


@functools.lru_cache(None)
def synth_gates():
    """exponent -> (the oracle's worst |value - ref64| over every case and row with that exponent, outside the excluded
    points; the gate: four times that, at least 2^-22)."""
    worst = {float(f32(e)): 0.0 for e in EXPS}                              # keyed by the fp32 exponent the kernel is handed
    for case in synth_cases():
        ref, margin, _ = synth_ref(case)
        err = np.where(margin >= MARGIN_SYNTH, np.abs(oracle_synth(case).astype(f64) - ref), 0.0)
        for b in range(SYNTH_B):
            e = synth_row_params(case, b)[1]
            worst[e] = max(worst[e], float(err[b].max()))
    return {e: (w, max(4.0 * w, 2.0 ** -22)) for e, w in worst.items()}


# ==== mx_interp_linear / _bwd ==================================================================================================
INTERP_PAIRS = ((2, 3), (345, 86410), (882, 345), (5, 5), (7, 1))
INTERP_ROWS = 3


def interp_windows(n_in, n_out):
    """name -> (j0, j_len): everything, the first output, the last output, a window strictly inside one input interval, a
    window over 2.5 input intervals (each as far as the size pair has one; duplicates dropped)."""
    scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    real = scale * np.arange(n_out)
    wins = {"all": (0, n_out), "first": (0, 1), "last": (n_out - 1, 1)}
    mid = (n_in - 1) // 2
    inside = np.nonzero((real > mid + 0.05) & (real < mid + 0.95))[0]
    if inside.size == 0:                                   # downsampling: a single output strictly between two inputs
        inside = np.nonzero(np.abs(real - np.round(real)) > 0.05)[0][:1]
    if inside.size:
        wins["inside_one_interval"] = (int(inside[0]), int(inside[-1] - inside[0] + 1))
    span = np.nonzero((real >= mid - 1 + 0.25) & (real <= mid + 1.75))[0]
    if span.size < 2 and n_out >= 3 and n_in > 3:          # downsampling: two neighbouring outputs span that much or more
        span = np.array([n_out // 2, n_out // 2 + 1])
    if span.size:
        wins["two_and_a_half_intervals"] = (int(span[0]), int(span[-1] - span[0] + 1))
    seen, out = set(), {}
    for k, w in wins.items():
        if w not in seen:
            seen.add(w)
            out[k] = w
    return out


def interp_dy(n_in, n_out, j0, j_len):
    return np.random.default_rng(1000 * n_in + n_out + 7 * j0 + j_len).standard_normal((INTERP_ROWS, j_len)).astype(f32)


@functools.lru_cache(None)
def interp_bwd_gate(n_in, n_out, j0, j_len):
    """(torch's fp32 autograd error against interp_bwd64 relative to max |dx_ref|, the gate: four times it, at least 1e-6)."""
    import torch
    import torch.nn.functional as F
    dy = interp_dy(n_in, n_out, j0, j_len)
    ref = L.interp_bwd64(dy, n_in, n_out, j0)
    x = torch.zeros(INTERP_ROWS, n_in, requires_grad=True)
    y = F.interpolate(x.unsqueeze(1), size=n_out, mode="linear", align_corners=True).squeeze(1) if n_in != n_out else x * 1.0
    g = torch.zeros(INTERP_ROWS, n_out)
    g[:, j0:j0 + j_len] = torch.from_numpy(dy)
    y.backward(g)
    err = float(np.abs(x.grad.numpy().astype(f64) - ref).max() / np.abs(ref).max())
    return err, max(4.0 * err, 1e-6)


# ==== corners ==================================================================================================================
CORNER_N = (9, 90, 345)
CORNER_R = (1, 63, 64, 65, 130)
MAX_N_CORNERS = (2, 6, 16)
GOOD_ROW = "alt2"             # one top, one bottom: valid under the default filter, stretched at every max_n_corners used here
VALID_GOOD_ROW = "count_2_3"  # accepted by every argument set of VALID_ARGS
VALID_ARGS = ((1, 6, 1, 6, 9), (2, 2, 1, 6, 9), (1, 6, 3, 3, 9), (1, 6, 1, 6, 0))
# the rows of the validity test (n = 90): counts 0, 1, 2, 6, 7 of either kind, smallest gaps 8, 9, 10, valid for tops only /
# for bottoms only; repeated so that every argument set accepts at least a quarter and rejects at least a quarter
VALID_ROWS = ("monotone", "one_top", "one_bottom", "count_1_1", "count_2_2", "count_6_6", "count_7_7", "count_7_6", "count_6_7",
              "count_1_6", "count_6_1", "count_2_6", "count_8_1", "count_1_8", "alt16", "alt17",
              "gap8_tops", "gap9_tops", "gap10_tops", "gap8_two_tops_one_bottom", "gap9_two_tops_one_bottom",
              "gap10_two_tops_one_bottom", "count_2_3", "count_2_3", "count_2_3", "gap9_tops", "gap10_tops", "gap10_tops")


def corner_stack(n, R, names=None, good=GOOD_ROW):
    """(rows (R, n) fp32, the designed case of every row): the designed rows repeated in a shuffled order; the first and the
    last row of every 64-row workgroup is ``good``."""
    d = L.designed_rows(n)
    names = list(d) if names is None else list(names)
    g = np.random.default_rng(n * 1000 + R)
    order = []
    while len(order) < R:
        order += [names[i] for i in g.permutation(len(names))]
    order = order[:R]
    for r in range(R):
        if r % 64 in (0, 63) or r == R - 1:
            order[r] = good
    return np.stack([d[k]["row"] for k in order]), order


def stretch_dout(n, R):
    return np.random.default_rng(n + 31 * R).standard_normal((R, n)).astype(f32)


@functools.lru_cache(None)
def stretch_bwd_gate(n, max_n_corners):
    """(oracle.modulations.stretch_corners_torch under fp32 autograd against stretch_bwd64, worst over the designed rows of
    length n with a finite gain, per row relative to max |dx_ref|; the gate: four times it, at least 1e-6)."""
    import torch
    from oracle import modulations as omod
    d = L.designed_rows(n)
    rows = np.stack([v["row"] for v in d.values()])
    rows = rows[L.stretch_gain_finite(rows, max_n_corners)]
    g = stretch_dout(n, len(rows))
    ref = L.stretch_bwd64(rows, g, max_n_corners)
    x = torch.from_numpy(rows).requires_grad_(True)
    omod.stretch_corners_torch(x, max_n_corners, 0).backward(torch.from_numpy(g))
    err = float((np.abs(x.grad.numpy().astype(f64) - ref).max(1) / np.abs(ref).max(1)).max())
    return err, max(4.0 * err, 1e-6)


SMOOTHEN_CASES = ((1, 1, 1), (3, 85, 1), (16, 16, 1), (1, 257, 1),           # (rows, n, k): rows (n - k + 1) in {1, 255, 256, 257}
                  (1, 2, 2), (3, 86, 2), (16, 17, 2), (1, 258, 2),
                  (1, 8, 8), (3, 92, 8), (16, 23, 8), (1, 264, 8),
                  (1, 9, 9), (255, 9, 9), (256, 9, 9), (257, 9, 9))

# ==== mx_lfo_loss ==============================================================================================================
LOSS_B = (1, 5, 65)
LOSS_N = (5, 6, 255, 256, 257, 345, 2047, 2048)
LOSS_W = ((1.0, 5.0, 10.0, 0.0), (0.0, 0.0, 0.0, 1.0), (1.0, 0.0, 2.0, 0.5), (1.0, -1.0, 0.0, 0.0))
MARGIN_LOSS, CAP_LOSS = 1e-6, 0.02
LOSS_AMPLITUDES = (1.0, 1e-4)


def loss_grid_inputs(B, n):
    """y_hat, y on multiples of 1 / 64: a third of the positions equal, a run with a constant error (first and second
    differences of the error vanish) and a run with a linear one (second differences vanish)."""
    g = np.random.default_rng(7 * B + n)
    y = g.integers(0, 65, (B, n))
    e = g.integers(-8, 9, (B, n))
    q = max(1, n // 4)
    e[:, :q] = 3
    e[:, q:2 * q] = np.arange(q) - 2
    rest = e[:, 2 * q:]
    rest[g.random(rest.shape) < 2.0 / 3.0] = 0
    return ((y + e) / 64.0).astype(f32), (y / 64.0).astype(f32)


def loss_generic_inputs(B, n, amplitude=1.0):
    """LFO-like rows (lfo_value64 of cos and tri, 0.5 to 3 periods per row) cast to fp32; y_hat = y + 1e-2 normal noise; both
    scaled by ``amplitude``."""
    g = np.random.default_rng(11 * B + n)
    y = np.stack([L.lfo_value64(L.lfo_arg32(np.arange(n), 0, g.uniform(0.5, 3.0), g.uniform(-math.pi, math.pi),
                                            (L.COS, L.TRI)[b % 2], float(n)), (L.COS, L.TRI)[b % 2])[0] for b in range(B)]).astype(f32)
    y_hat = (y + 1e-2 * g.standard_normal((B, n))).astype(f32)
    return (y_hat * f32(amplitude)).astype(f32), (y * f32(amplitude)).astype(f32)


def oracle_loss_error(y_hat, y, w):
    """oracle.losses in fp32 against lfo_loss64: the relative error of the four terms and the total (5,)."""
    import torch
    from oracle import losses as olosses
    ref = L.lfo_loss64(y_hat, y, w)
    a, t = torch.from_numpy(y_hat), torch.from_numpy(y)
    n = y_hat.shape[1]
    terms = [float(olosses.get_loss_func_by_name(k)(a, t)) if n > lo else 0.0 for k, lo in (("l1", 0), ("fdl1", 2), ("sdl1", 4), ("mse", 0))]
    total = float(sum(f32(wk) * f32(tk) for wk, tk in zip(w, terms) if wk > 0))
    want = np.append(ref["terms"], ref["total"])
    return np.abs(np.append(terms, total) - want) / np.maximum(np.abs(want), 1e-300)

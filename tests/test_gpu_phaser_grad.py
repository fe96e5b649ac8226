"""GPU: the differentiable phaser (mx_phaser_fwd_stash + mx_phaser_bwd, fx.PhaserModule) against the fp64 explicit adjoint of
tests/helpers/phaser_adjoint64.py.

Grid: centre {70, 440, 5 000, 18 000} Hz x feedback {-0.7, 0, 0.25, 0.7, 0.95} x depth {0.2, 1} x mix {0.2, 1} = 80 clips of
2 s + 0.5 s lead, once with the built-in oscillator and once with an external LFO of the six continuous shapes, rates
0.8 .. 2.8 Hz (whole periods in 2.5 s, so that the share of clamped groups is that of the shape: inv_rect_cos at 5 / 18 kHz
and rect_cos at 70 Hz would clamp more than half of their groups and are replaced by cos / tri there).  Input gain 0.3 (chosen on the CPU
with the helper: at most 16 % of a case's samples clip, at 0.35 it is 19.5 %, at 0.45 26 %; the resonance at feedback 0.95
sets it): some outputs clip.  Conditions asserted per case: <= 20 % of the samples clipped, <= 50 % of the groups clamped; some case has
both.  Samples whose fp32 m lies within 1 ulp of +-1 and groups whose pre lies within 1 ulp of 0 or 1 are left out of the
comparison of their own gradient entry (their number is printed and stays under 0.1 % of the case).

What is compared is the gradient of the forward that was differentiated: the helper is evaluated at the output-clip
decisions the stash forward took (read from the stash).  The scan's y is within 1e-5 of the sequential fp32 forward's up to
|feedback| 0.7 and within 6e-5 at 0.95 (re-association of its chunk maps, amplified by 1 / (1 - fb)), so a sample whose m lies
that close to +-1 can be clipped by one and not by the other -- far more than the 1 ulp the exclusion rule covers.  check()
prints how many decisions differ (ONE sample of the external-LFO grid, of 16 x 88 200 at feedback 0.95; none elsewhere),
asserts that each lies within the forward's bound of the edge, and prints the comparison at the sequential forward's
decisions for information (that one case: dx 1.71e-3, d centre 1.76e-3, d mix 1.28e-3 -- the gradient of another function).

Gates: every gradient is compared norm-wise over a batch, max |g - g64| / max |g64|, separately for |feedback| <= 0.7 and
above; GATES holds, per quantity, 10x the worst value measured on one MI355X (profiles/r07/measured_errors_gpu_tests.json;
every gate prints what it measures).  Measured: |feedback| <= 0.7: dx 2.25e-5, dmod 3.87e-5, parameters 1.71e-5;
feedback 0.95: dx 1.08e-4, dmod 1.28e-4, parameters 3.39e-4 (d mix of a 4 s clip).  The second bucket is looser and above
1e-4; the cause: the forward's coefficients are fp32 (G differs from the fp64 chain by up to 1.5e-6 relative) and so are
the states the backward recomputes, and the resonance at 0.95 amplifies both.  On the CPU, the fp64 adjoint of that 4 s
clip (another random dy) moves by 2.5e-4 in d mix with the fp32-rounded G alone and by 2.8e-4 with fp32 G and an fp32
forward (profiles/r07/README.md); on the 2 s grid fp32 G alone gives dx 2.2e-5, dmod 1.9e-4, d feedback 8.8e-5.
"""
import math

import numpy as np
import pytest
import torch

from tests.helpers import phaser_adjoint64 as pa

pytestmark = pytest.mark.gpu
SR = 44100.0
SHAPES = ["cos", "rect_cos", "inv_rect_cos", "tri", "saw", "rsaw"]
PARAMS = pa.PARAMS
# 10x the worst measured value (in brackets): lo = |feedback| <= 0.7, hi = 0.9 / 0.95; param = the four fp64-summed parameter
# gradients.  Every case is held to these, whether or not one of its clip decisions differs.
GATES = {"dx_lo": 2.3e-4,     # [2.25e-5]
         "dmod_lo": 3.9e-4,   # [3.87e-5]
         "param_lo": 1.8e-4,  # [1.71e-5]
         "dx_hi": 1.1e-3,     # [1.08e-4]
         "dmod_hi": 1.3e-3,   # [1.28e-4]
         "param_hi": 3.4e-3}  # [3.39e-4]

def audio_np(B, T, seed, gain):
    g = np.random.default_rng(seed)
    t = np.arange(T) / SR
    x = 0.5 * np.sin(2 * math.pi * 220.0 * t)[None, :] + g.uniform(-0.4, 0.4, (B, T))
    return (gain * x).astype(np.float32)


def lfo_np(shape, n, rate, phase):
    """the six continuous shapes at group rate (sr / 4), values in [0, 1]"""
    ph = (2 * math.pi * rate * np.arange(n) * 4 / SR + phase) % (2 * math.pi)
    u = ph / (2 * math.pi)
    y = {"cos": (np.cos(ph) + 1) / 2, "rect_cos": np.abs(np.cos(ph / 2)), "inv_rect_cos": 1 - np.abs(np.cos(ph / 2)),
         "tri": 1 - np.abs(2 * u - 1), "saw": u, "rsaw": 1 - u}[shape]
    return y.astype(np.float32)


def grid_params():
    combos = [(c, fb, d, mx) for c in (70.0, 440.0, 5000.0, 18000.0) for fb in (-0.7, 0.0, 0.25, 0.7, 0.95)
              for d in (0.2, 1.0) for mx in (0.2, 1.0)]
    cols = list(zip(*combos))
    return {k: np.asarray(v, np.float32) for k, v in zip(("centre_frequency_hz", "feedback", "depth", "mix"), cols)}


def grid_rates(B):
    return np.asarray([0.8 + 0.4 * (i % 6) for i in range(B)], np.float32)


def grid_mod(params, T, seed):
    g = np.random.default_rng(seed)
    B, ng = len(params["mix"]), (T + 3) // 4
    rows = []
    for i in range(B):
        shape = SHAPES[i % 6]
        c = float(params["centre_frequency_hz"][i])
        if c >= 5000.0 and shape == "inv_rect_cos":
            shape = "cos"
        if c == 70.0 and shape == "rect_cos":
            shape = "tri"
        rate = float(grid_rates(B)[i]) * (2.0 if "rect" in shape else 1.0)      # rectified cosines: half rate inside
        rows.append(lfo_np(shape, ng, rate, float(g.uniform(0, 2 * math.pi))))
    return np.stack(rows)


def dev_params(dev, params, rate=None):
    p = {k: torch.tensor(v, device=dev) for k, v in params.items()}
    if rate is not None:
        p["rate_hz"] = torch.tensor(rate, device=dev)
    return p


def normwise(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def ulp_edges(ref):
    """(samples whose fp32 m is within 1 ulp of +-1, groups whose pre is within 1 ulp of 0 or 1)"""
    m, pre = ref["fwd32"]["m"], ref["fwd32"]["pre"]
    one = np.float32(1.0)
    near_m = np.abs(np.abs(m) - one) <= np.spacing(one)
    near_p = (np.abs(pre) <= np.float32(1.5e-45)) | (np.abs(pre - one) <= np.spacing(one))
    return near_m, near_p


def gpu_decisions(st, width, T):
    """The output-clip decisions the stash forward took (csrc/phaser_common.h): (B, T) bool."""
    from mod_extraction_amd import fx
    sg, _ = fx.phaser_stash_shape(width)
    bits = st.view(torch.int32)[:, 3 * sg:4 * sg].cpu().numpy()
    return (((bits[:, :, None] >> np.arange(4)[None, None, :]) & 1) != 0).reshape(bits.shape[0], -1)[:, :T]


def errors(ref, fb, sel, dx, dmod, g, keep_x, keep_g):
    out = {}
    for bucket, msk in (("lo", np.abs(fb) <= 0.7), ("hi", np.abs(fb) > 0.7)):
        if not msk.any():
            continue
        if dx is not None:
            a, b = dx.cpu().numpy()[sel][msk], ref["dx"][msk]
            out["dx_" + bucket] = normwise(np.where(keep_x[msk], a, 0.0), np.where(keep_x[msk], b, 0.0))
        if dmod is not None:
            ng = ref["dmod"].shape[1]
            a, b = dmod.cpu().numpy()[sel][msk][:, :ng], ref["dmod"][msk]
            out["dmod_" + bucket] = normwise(np.where(keep_g[msk], a, 0.0), np.where(keep_g[msk], b, 0.0))
        for k in PARAMS:
            if k in g:
                out[f"{k}_{bucket}"] = normwise(g[k].cpu().numpy()[sel][msk], ref[k][msk])
    return out


def gate_of(k):
    return k if k.startswith(("dx", "dmod")) else "param_" + k[-2:]


def check(tag, ref, fbs, y, dx, dmod, g, lead, again, rows=None, forward_exact=False):
    """Compare one launch's results (tensors over all B rows) with the fp64 helper's on the rows ``rows``.
    again = (stash, source width, function pass_m -> helper result).  The gradient compared is that of the forward that was
    differentiated: the helper is evaluated at the output-clip decisions the stash forward took (read from the stash).
    They differ from the sequential fp32 forward's only where the scan's y does, i.e. for samples whose m lies within the
    forward's own error of +-1; the number of such samples is printed and each is asserted to lie that close to the edge.
    The comparison at the helper's own decisions is printed for information when there are any."""
    sel = np.arange(len(fbs)) if rows is None else np.asarray(rows)
    fb = fbs[sel]
    near_m, near_p = ulp_edges(ref)
    n_m, n_p = int(near_m.sum()), int(near_p.sum())
    print(f"{tag}: left out {n_m} samples near the clip edge, {n_p} groups near the clamp edge")
    assert n_m <= 1e-3 * near_m.size and n_p <= 1e-3 * near_p.size
    yh = y.cpu().numpy()[sel]
    y32 = ref["fwd32"]["y"][:, lead:]
    # the project's waveform criterion, 1e-5 of the peak, holds up to |feedback| 0.7 (DESIGN K3: 4.4e-6 there); the
    # chunk-start states carry the maps' re-association error, which the loop amplifies by 1 / (1 - |fb|): at 0.95 the
    # bound is 1e-5 * (1 - 0.7) / (1 - 0.95) = 6e-5.  (This is the parent's forward, bit for bit; not this file's subject.)
    fwd_bound = np.where(np.abs(fb) <= 0.7, 1e-5, 6e-5)
    if forward_exact:
        assert np.array_equal(yh, y32)
    else:
        for bound in (1e-5, 6e-5):
            msk = fwd_bound == bound
            if msk.any():
                e = float(np.abs(yh[msk] - y32[msk]).max() / np.abs(y32[msk]).max())
                print(f"{tag}: forward {e:.3e} (bound {bound:.0e})")
                assert e < bound
    st, width, recompute = again
    mine = gpu_decisions(st, width, ref["pass_m"].shape[1])[sel]
    flipped = mine != ref["pass_m"]
    flips = int(flipped.sum())
    print(f"{tag}: {flips} output-clip decisions differ between the scan forward and the sequential fp32 forward")
    # an entry is left out where ITS OWN mask decision sits within 1 ulp of an edge
    keep_x, keep_g = ~near_m, ~near_p
    at_mine = ref
    if flips:
        dist = np.abs(np.abs(ref["fwd32"]["m"].astype(np.float64)) - 1.0)
        peak = np.maximum(np.abs(ref["fwd32"]["y"]).max(1), 1.0)
        assert (dist[flipped] <= (fwd_bound * peak)[np.nonzero(flipped)[0]]).all()      # only samples that close to +-1
        print(tag, "at the sequential forward's decisions (information)",
              {k: f"{v:.2e}" for k, v in errors(ref, fb, sel, dx, dmod, g, keep_x, keep_g).items()})
        at_mine = recompute(mine)
    out = errors(at_mine, fb, sel, dx, dmod, g, keep_x, keep_g)
    print(tag, {k: f"{v:.2e}" for k, v in out.items()})
    for k, v in out.items():
        assert v < GATES[gate_of(k)], (tag, k, v)
    return out


def run(dev, x, p, lead, n, mod=None, rows=None, **kw):
    from mod_extraction_amd import fx
    lead_t = torch.full((x.size(0),), lead, device=dev, dtype=torch.int32)
    y, st = fx.phaser_forward_stash(x, p, lead_t, SR, n, mod=mod, rows=rows)
    return (y, st, lead_t)


def reference(x_np, osc, params, lead, dy_np, with_recompute=False):
    dy_full = np.concatenate([np.zeros((x_np.shape[0], lead)), dy_np.astype(np.float64)], 1)
    ref = pa.phaser_adjoint64(x_np, osc, params, SR, dy_full)
    if with_recompute:
        return ref, lambda pass_m: pa.phaser_adjoint64(x_np, osc, params, SR, dy_full, fwd32=ref["fwd32"], pass_m=pass_m)
    return ref


def test_apply_effect_is_differentiable(dev):
    """Fails without the feature (no PhaserModule): apply_effect on an x that requires grad returns a y with a grad_fn,
    bit-identical to phaser_forward, and y.sum().backward() fills x.grad on lead and window samples alike."""
    from mod_extraction_amd import fx
    B, lead, n = 3, 4410, 22050
    m = fx.PhaserModule(SR)
    x = torch.tensor(audio_np(B, lead + n, 1, 0.8), device=dev).unsqueeze(1).requires_grad_(True)
    rate = torch.tensor([0.7, 1.5, 3.0], device=dev)
    y = m.apply_effect(x, rate_hz=rate, depth=0.9, centre_frequency_hz=800.0, feedback=0.6, mix=0.7, lead=lead)
    assert y.grad_fn is not None and y.shape == (B, 1, n)
    p = {"rate_hz": rate, "depth": torch.full((B,), 0.9, device=dev), "centre_frequency_hz": torch.full((B,), 800.0, device=dev),
         "feedback": torch.full((B,), 0.6, device=dev), "mix": torch.full((B,), 0.7, device=dev)}
    y0 = fx.phaser_forward(x.detach()[:, 0], p, torch.full((B,), lead, device=dev, dtype=torch.int32), SR, n)
    assert torch.equal(y.detach()[:, 0], y0)
    assert torch.equal(m(x.detach(), rate_hz=rate, depth=0.9, centre_frequency_hz=800.0, feedback=0.6, mix=0.7, lead=lead), y.detach())
    y.sum().backward()
    gx = x.grad[:, 0]
    assert torch.isfinite(gx).all() and gx[:, :lead].abs().sum() > 0 and gx[:, lead:].abs().sum() > 0
    with torch.no_grad():
        assert m.apply_effect(x, rate_hz=rate, depth=0.9, feedback=0.6, lead=lead).grad_fn is None
    with pytest.raises(ValueError):
        m.apply_effect(x, rate_hz=rate.clone().requires_grad_(True), lead=lead)
    with pytest.raises(AssertionError):
        m.apply_effect(x, rate_hz=rate, mod_sig=torch.zeros(B, lead + n, device=dev), lead=lead)


def test_external_lfo_forward(dev):
    """Fails without the feature: the stash forward driven by a saw and a triangle against the helper's fp32 forward; with
    mod = None bit-identical to mx_phaser_fwd incl. dry_out, a rows subset and strided rows."""
    from mod_extraction_amd import fx
    B, lead, n = 4, 8820, 88200
    T = lead + n
    ng = (T + 3) // 4
    x_np = audio_np(B, T, 2, 0.7)
    mod_np = np.stack([lfo_np(s, ng, r, ph) for s, r, ph in (("saw", 1.3, 0.4), ("tri", 2.1, 1.0), ("saw", 0.6, 2.0), ("tri", 3.0, 0.0))])
    params = {"depth": np.asarray([1.0, 0.7, 0.5, 1.0], np.float32), "centre_frequency_hz": np.asarray([440.0, 1300.0, 3000.0, 200.0], np.float32),
              "feedback": np.asarray([0.7, 0.0, -0.7, 0.5], np.float32), "mix": np.asarray([0.5, 1.0, 0.7, 1.0], np.float32)}
    x = torch.tensor(x_np, device=dev)
    lead_t = torch.full((B,), lead, device=dev, dtype=torch.int32)
    y, _ = fx.phaser_forward_stash(x, dev_params(dev, params), lead_t, SR, n, mod=torch.tensor(mod_np, device=dev))
    osc = (np.float32(1.0) - np.float32(2.0) * mod_np).astype(np.float32)
    y32 = pa.forward32(x_np, osc, params, SR)["y"][:, lead:]
    e = float(np.abs(y.cpu().numpy() - y32).max() / np.abs(y32).max())
    print(f"external LFO forward: max |y - y32| / max |y32| = {e:.3e}")
    assert e < 1e-5
    # mod = None: the built-in oscillator, bit-identical to mx_phaser_fwd; strided rows (one channel of (B, 2, T)), rows subset
    p = dev_params(dev, params, np.asarray([0.5, 1.0, 2.0, 3.0], np.float32))
    xx = torch.tensor(audio_np(2 * B, T, 3, 0.7), device=dev).view(B, 2, T)
    xs = xx[:, 1]
    rows = torch.tensor([3, 1], device=dev, dtype=torch.int32)
    for r in (None, rows):
        y0, d0 = torch.full((B, n), 7.0, device=dev), torch.full((B, n), 7.0, device=dev)
        y1, d1 = torch.full((B, n), 7.0, device=dev), torch.full((B, n), 7.0, device=dev)
        fx.phaser_forward(xs, p, lead_t, SR, n, rows=r, out=y0, dry_out=d0)
        fx.phaser_forward_stash(xs, p, lead_t, SR, n, rows=r, out=y1, dry_out=d1)
        assert torch.equal(y0, y1) and torch.equal(d0, d1)
        if r is not None:
            assert (y1[[0, 2]] == 7.0).all() and (y1[[1, 3]] != 7.0).any()


@pytest.mark.parametrize("lfo", ["builtin", "external"])
def test_grid_matches_fp64(dev, lfo):
    from mod_extraction_amd import fx
    params = grid_params()
    B, lead, n = len(params["mix"]), 22050, 88200
    T = lead + n
    x_np = audio_np(B, T, 11, 0.3)
    if lfo == "builtin":
        rate = grid_rates(B)
        osc, _ = pa.builtin_osc(rate, (T + 3) // 4, SR)
        mod, p = None, dev_params(dev, params, rate)
    else:
        mod_np = grid_mod(params, T, 12)
        osc = (np.float32(1.0) - np.float32(2.0) * mod_np).astype(np.float32)
        mod, p = torch.tensor(mod_np, device=dev), dev_params(dev, params)
    dy = torch.randn(B, n, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    x = torch.tensor(x_np, device=dev)
    y, st, lead_t = run(dev, x, p, lead, n, mod=mod)
    dx, dmod, g = fx.phaser_backward(dy, x, st, p, lead_t, SR, n)
    ref, recompute = reference(x_np, osc, params, lead, dy.cpu().numpy(), with_recompute=True)
    clipped = (~ref["pass_m"]).mean(1)
    clamped = (~ref["inside"]).mean(1)
    print(f"{lfo}: clipped samples per case max {clipped.max():.3f}, clamped groups per case max {clamped.max():.3f}")
    assert clipped.max() <= 0.20 and clamped.max() <= 0.50
    assert ((clipped > 0) & (clamped > 0)).any()
    check("grid " + lfo, ref, params["feedback"], y, dx, dmod, g, lead, again=(st, T, recompute))


def test_long_clips_rows_subset_strides_null_outputs(dev):
    """4 s clips; a rows subset leaves the other rows untouched (their parameter gradients 0); strided dx; NULL outputs;
    params_wanted = ("mix",)."""
    from mod_extraction_amd import fx
    B, lead, n = 6, 11025, 176400
    T = lead + n
    params = {k: v[[5, 27, 38, 44, 61, 79]] for k, v in grid_params().items()}
    params["centre_frequency_hz"] = np.asarray([440.0, 440.0, 1300.0, 5000.0, 5000.0, 800.0], np.float32)
    x_np = audio_np(B, T, 21, 1.1)
    mod_np = np.stack([lfo_np(SHAPES[i], (T + 3) // 4, 0.5 + 0.5 * i, 0.3 * i) for i in range(B)])
    x, mod, p = torch.tensor(x_np, device=dev), torch.tensor(mod_np, device=dev), dev_params(dev, params)
    dy = torch.randn(B, n, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    sel = [5, 0, 3]
    rows = torch.tensor(sel, device=dev, dtype=torch.int32)
    lead_t = torch.full((B,), lead, device=dev, dtype=torch.int32)
    y = torch.full((B, n), 7.0, device=dev)
    y, st = fx.phaser_forward_stash(x, p, lead_t, SR, n, mod=mod, rows=rows, out=y)
    dxx = torch.full((B, 2, T), 7.0, device=dev)
    dm = torch.full((B, (T + 3) // 4), 7.0, device=dev)
    dx, dmod, g = fx.phaser_backward(dy, x, st, p, lead_t, SR, n, rows=rows, dx=dxx[:, 1], dmod=dm)
    untouched = [1, 2, 4]
    assert (y[untouched] == 7.0).all() and (dxx[untouched] == 7.0).all() and (dm[untouched] == 7.0).all()
    assert (dxx[:, 0] == 7.0).all()
    assert all((g[k][untouched] == 0).all() for k in PARAMS)
    osc = (np.float32(1.0) - np.float32(2.0) * mod_np).astype(np.float32)
    ref, recompute = reference(x_np[sel], osc[sel], {k: v[sel] for k, v in params.items()}, lead, dy.cpu().numpy()[sel], True)
    check("4 s rows subset", ref, params["feedback"], y, dx, dmod, g, lead, rows=sel, again=(st, T, recompute))
    # NULL outputs and a single parameter: the same bits
    dx2, dmod2, g2 = fx.phaser_backward(dy, x, st, p, lead_t, SR, n, rows=rows, need_dmod=False, params_wanted=("mix",))
    assert dmod2 is None and set(g2) == {"mix"} and torch.equal(g2["mix"], g["mix"])
    assert torch.equal(dx2[sel], dx[sel])
    dx3, dmod3, g3 = fx.phaser_backward(dy, x, st, p, lead_t, SR, n, rows=rows, need_dx=False, params_wanted=())
    assert dx3 is None and g3 == {} and torch.equal(dmod3[sel], dmod[sel])


def test_backward_is_deterministic(dev):
    from mod_extraction_amd import fx
    params = grid_params()
    B, lead, n = len(params["mix"]), 22050, 88200
    x = torch.tensor(audio_np(B, lead + n, 31, 1.1), device=dev)
    p = dev_params(dev, params, grid_rates(B))
    dy = torch.randn(B, n, device=dev)
    res = []
    for _ in range(2):
        y, st, lead_t = run(dev, x, p, lead, n)
        dx, dmod, g = fx.phaser_backward(dy, x, st, p, lead_t, SR, n)
        res.append((y, dx, dmod, g))                       # (the stash has padding that nobody writes: not compared)
    a, b = res
    assert all(torch.equal(a[i], b[i]) for i in range(3)) and all(torch.equal(a[3][k], b[3][k]) for k in PARAMS)


def test_multichannel_and_mixed_params(dev):
    """n_ch = 2, a full-rate mod_sig shared by the channels, per-clip leads, float and tensor parameters mixed: tensor
    parameters get (B,) gradients summed over the channels, python floats None."""
    from mod_extraction_amd import fx
    B, W = 3, 44100
    leads = [0, 2205, 4410]
    n = W - max(leads)
    m = fx.PhaserModule(SR)
    x = torch.tensor(audio_np(2 * B, W, 41, 1.1), device=dev).view(B, 2, W).requires_grad_(True)
    t = torch.arange(W, device=dev) / SR
    mod = (0.5 + 0.5 * torch.sin(2 * math.pi * torch.tensor([1.0, 2.0, 3.0], device=dev)[:, None] * t[None, :])).requires_grad_(True)
    fb = torch.tensor([0.3, -0.7, 0.9], device=dev, requires_grad=True)
    centre = torch.tensor([440.0, 1300.0, 3000.0], device=dev, requires_grad=True)
    depth = torch.tensor([0.8, 0.5, 1.0], device=dev)                          # a tensor that does not require grad
    y = m.apply_effect(x, mod_sig=mod, depth=depth, centre_frequency_hz=centre, feedback=fb, mix=0.75,
                       lead=torch.tensor(leads, device=dev))
    assert y.shape == (B, 2, n)
    dy = torch.randn_like(y)
    (y * dy).sum().backward()
    assert depth.grad is None
    assert (mod.grad[:, 1::4] == 0).all() and (mod.grad[:, 2::4] == 0).all()    # only samples 0, 4, 8, ... drive the cut-off
    # the clip decisions of the forward that was differentiated: the same launch once more, for its stash
    with torch.no_grad():
        rows_p = {"depth": depth.repeat_interleave(2), "centre_frequency_hz": centre.detach().repeat_interleave(2),
                  "feedback": fb.detach().repeat_interleave(2), "mix": torch.full((2 * B,), 0.75, device=dev)}
        y_rows, st = fx.phaser_forward_stash(x.detach().reshape(2 * B, W), rows_p,
                                             torch.tensor(leads, device=dev, dtype=torch.int32).repeat_interleave(2), SR, n,
                                             mod=mod.detach()[:, ::4].repeat_interleave(2, 0).contiguous())
    assert torch.equal(y_rows.view(B, 2, n), y.detach())
    decisions = gpu_decisions(st, W, W)
    for b in range(B):                                                         # per clip: its own lead, both channels
        T = leads[b] + n
        xb = x.detach()[b].cpu().numpy()[:, :T]
        mb = mod.detach()[b].cpu().numpy()[::4][:(T + 3) // 4]
        osc = np.repeat((np.float32(1.0) - np.float32(2.0) * mb)[None, :], 2, 0).astype(np.float32)
        pr = {"depth": np.full(2, float(depth[b]), np.float32), "centre_frequency_hz": np.full(2, float(centre[b]), np.float32),
              "feedback": np.full(2, float(fb[b]), np.float32), "mix": np.full(2, 0.75, np.float32)}
        ref, recompute = reference(xb, osc, pr, leads[b], dy[b].cpu().numpy(), with_recompute=True)
        mine = decisions[2 * b:2 * b + 2, :T]
        flips = int((mine != ref["pass_m"]).sum())
        print(f"n_ch = 2, clip {b}: {flips} output-clip decisions differ from the sequential fp32 forward's")
        if flips:
            ref = recompute(mine)
        gx = x.grad[b].cpu().numpy()
        assert (gx[:, T:] == 0).all()
        e = {"dx": normwise(gx[:, :T], ref["dx"]),
             "dmod": normwise(mod.grad[b].cpu().numpy()[::4][:(T + 3) // 4], ref["dmod"].sum(0)),
             "feedback": normwise(fb.grad[b].cpu().numpy(), ref["feedback"].sum()),
             "centre": normwise(centre.grad[b].cpu().numpy(), ref["centre_frequency_hz"].sum())}
        print("n_ch = 2, clip", b, {k: f"{v:.2e}" for k, v in e.items()})
        hi = abs(float(fb[b])) > 0.7
        assert e["dx"] < GATES["dx_hi" if hi else "dx_lo"] and e["dmod"] < GATES["dmod_hi" if hi else "dmod_lo"]
        assert max(e["feedback"], e["centre"]) < GATES["param_hi" if hi else "param_lo"]


def test_full_batch_256x4s(dev):
    """256 clips x (4 s + lead), built-in oscillator; a sampled subset against the fp64 adjoint."""
    from mod_extraction_amd import fx
    B, lead, n = 256, 14700, 176400
    T = lead + n
    gp = grid_params()
    params = {k: np.tile(v, 4)[:B] for k, v in gp.items()}
    rate = np.tile(grid_rates(80), 4)[:B]
    x_np = audio_np(B, T, 51, 1.1)
    x, p = torch.tensor(x_np, device=dev), dev_params(dev, params, rate)
    dy = torch.randn(B, n, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    y, st, lead_t = run(dev, x, p, lead, n)
    dx, dmod, g = fx.phaser_backward(dy, x, st, p, lead_t, SR, n)
    assert torch.isfinite(dx).all() and torch.isfinite(dmod).all() and all(torch.isfinite(v).all() for v in g.values())
    sel = [0, 37, 101, 176, 255]
    osc, _ = pa.builtin_osc(rate[sel], (T + 3) // 4, SR)
    ref, recompute = reference(x_np[sel], osc, {k: v[sel] for k, v in params.items()}, lead, dy.cpu().numpy()[sel], True)
    check("256 x 4 s", ref, params["feedback"], y, dx, dmod, g, lead, rows=sel, again=(st, T, recompute))


@pytest.mark.parametrize("total", [1, 3, 4, 5, 2047, 2048, 2049])
def test_lengths_around_the_tiling(dev, total):
    """Fewer groups than lanes, a last group that is not full: lead + N = total with lead = total // 3."""
    from mod_extraction_amd import fx
    B = 4
    lead = total // 3
    n = total - lead
    W = total + 5                                                              # a source row wider than the clip
    params = {k: v[[9, 30, 46, 77]] for k, v in grid_params().items()}
    params["centre_frequency_hz"] = np.asarray([440.0, 1300.0, 5000.0, 800.0], np.float32)
    x_np = audio_np(B, W, 60 + total, 1.1)
    ngw = (W + 3) // 4
    mod_np = np.stack([lfo_np(SHAPES[i], ngw, 40.0 * (i + 1), 0.5 * i) for i in range(B)])
    x, mod, p = torch.tensor(x_np, device=dev), torch.tensor(mod_np, device=dev), dev_params(dev, params)
    dy = torch.randn(B, n, device=dev, generator=torch.Generator(device=dev).manual_seed(total))
    lead_t = torch.full((B,), lead, device=dev, dtype=torch.int32)
    y, st = fx.phaser_forward_stash(x, p, lead_t, SR, n, mod=mod)
    dx, dmod, g = fx.phaser_backward(dy, x, st, p, lead_t, SR, n)
    ng = (total + 3) // 4
    assert (dx[:, total:] == 0).all() and (dmod[:, ng:] == 0).all()
    osc = (np.float32(1.0) - np.float32(2.0) * mod_np[:, :ng]).astype(np.float32)
    ref, recompute = reference(x_np[:, :total], osc, params, lead, dy.cpu().numpy(), True)
    check(f"total {total}", ref, params["feedback"], y, dx[:, :total], dmod, g, lead, forward_exact=total <= 5,
          again=(st, W, recompute))


@pytest.mark.parametrize("total,W", [(5, 10), (1000, 1000), (2049, 2049), (3000, 9001)])
def test_stash_row_is_written_whole(dev, total, W):
    """mx_phaser_fwd_stash defines every word of a stash row (csrc/phaser_common.h: ps_stash_floats(sg)), whatever the buffer
    held: the group records beyond the clip's groups, the pad float of every chunk map, the checkpoint slots of chunks without
    a group and those beyond the clip's own packing are zeros.  Clips shorter than their row (per-clip lead-ins below the
    row's) leave most of the row to this rule; (3000, 9001) has 750 of 2252 groups and 2 of 5 groups per chunk in use."""
    from mod_extraction_amd import fx
    B = 3
    leads = [total // 3, 0, total // 2]
    n = total - max(leads)
    params = {k: v[[9, 30, 46]] for k, v in grid_params().items()}
    params["centre_frequency_hz"] = np.asarray([440.0, 1300.0, 5000.0], np.float32)
    ngw = (W + 3) // 4
    x = torch.tensor(audio_np(B, W, 90 + total, 0.9), device=dev)
    mod = torch.tensor(np.stack([lfo_np(SHAPES[i], ngw, 40.0 * (i + 1), 0.5 * i) for i in range(B)]), device=dev)
    p, lead_t = dev_params(dev, params), torch.tensor(leads, device=dev, dtype=torch.int32)
    sg, row = fx.phaser_stash_shape(W)
    got = []
    for fill in (float("nan"), 7.0):
        y, st = fx.phaser_forward_stash(x, p, lead_t, SR, n, mod=mod, stash=torch.full((B, row), fill, device=dev))
        got.append((y.cpu(), st.cpu()))
    assert not torch.isnan(got[0][1]).any()
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    st = got[0][1].numpy()
    P, MV = 512, 57                                                            # PS_P, PS_MV of csrc/phaser_common.h
    for b in range(B):
        n_groups = (leads[b] + n + 3) // 4
        for section in range(4):
            assert (st[b, section * sg + n_groups:(section + 1) * sg].view(np.int32) == 0).all(), (b, section)
        maps = st[b, 4 * sg:4 * sg + P * MV].reshape(P, MV)
        assert (maps[:, MV - 1].view(np.int32) == 0).all()
        gpc = -(-n_groups // P)
        spc = -(-gpc // 2)
        ck = st[b, 4 * sg + P * MV:]
        assert ck.size == P * 8 * (-(-(-(-sg // P)) // 2))
        used = ck[:P * spc * 8].reshape(P, spc, 8)
        for chunk in range(P):
            g0 = min(chunk * gpc, n_groups)
            live = -(-(min(g0 + gpc, n_groups) - g0) // 2)
            assert (used[chunk, live:].view(np.int32) == 0).all(), (b, chunk)
        assert (ck[P * spc * 8:].view(np.int32) == 0).all(), b
    # the adjoint reads the same bits from either row
    dy = torch.randn(B, n, device=dev, generator=torch.Generator(device=dev).manual_seed(total))
    outs = []
    for _, st_h in got:
        dx, dmod, g = fx.phaser_backward(dy, x, st_h.to(dev), p, lead_t, SR, n)
        outs.append([dx.cpu(), dmod.cpu()] + [g[k].cpu() for k in sorted(g)])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_fit_by_analysis_by_synthesis(dev):
    """End to end.  4 clips x 0.5 s of three partials (220 / 330 / 440 Hz), a phaser driven by a 2 Hz LFO built from torch
    ops at group rate, mod = (1 + sin(2 pi 2 t + phase)) / 2, the phase a learnable parameter.  Targets: feedback 0.5, depth
    0.7, centre 1000 Hz (fitted as norm_centre = log10(centre / 20) / log10(1000), true value 0.5663), phase 1.0; mix 0.8
    fixed.  Adam (lr 0.02 decaying to 2e-4 over 500 steps) on the L1 loss through apply_effect from feedback, depth and phase
    0.2 away and norm_centre 0.1 away.  The loss must fall >= 100x and every parameter end within 0.02 of its true value
    (the flanger test's thresholds).  The same fit with the fp64 helper's gradient at 0.1 s converges on the CPU
    (profiles/r07/README.md)."""
    from mod_extraction_amd import fx
    B, N = 4, 22050
    m = fx.PhaserModule(SR)
    t = (torch.arange(N, device=dev) / SR).float()
    x = (0.3 * torch.sin(2 * math.pi * 220.0 * t) + 0.2 * torch.sin(2 * math.pi * 330.0 * t + 1.0) +
         0.15 * torch.sin(2 * math.pi * 440.0 * t + 2.0)).expand(B, N).unsqueeze(1).contiguous()
    x = x * torch.linspace(0.8, 1.2, B, device=dev).view(B, 1, 1)
    tg = t[::4]
    log_span = math.log10(1000.0)
    true = {"fb": 0.5, "depth": 0.7, "nc": math.log10(1000.0 / 20.0) / log_span, "phase": 1.0}

    def render(fb, depth, nc, phase):
        mod = (1.0 + torch.sin(2 * math.pi * 2.0 * tg[None, :] + phase[:, None])) / 2.0
        centre = 20.0 * 10.0 ** (nc * log_span)
        return m.apply_effect(x, mod_sig=mod, depth=depth, centre_frequency_hz=centre, feedback=fb, mix=0.8)

    with torch.no_grad():
        target = render(*(torch.full((B,), true[k], device=dev) for k in ("fb", "depth", "nc", "phase")))
    start = {"fb": 0.3, "depth": 0.5, "nc": true["nc"] - 0.1, "phase": 0.8}
    p = {k: torch.full((B,), v, device=dev, requires_grad=True) for k, v in start.items()}
    opt = torch.optim.Adam(p.values(), lr=0.02)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.01 ** (1 / 500))
    losses = []
    for _ in range(500):
        opt.zero_grad()
        loss = (render(p["fb"], p["depth"], p["nc"], p["phase"]) - target).abs().mean()
        loss.backward()
        opt.step()
        sched.step()
        with torch.no_grad():
            p["fb"].clamp_(-0.95, 0.95)
            p["depth"].clamp_(0.0, 1.0)
            p["nc"].clamp_(0.05, 0.95)
        losses.append(float(loss))
    print("loss", losses[0], losses[-1], {k: v.detach().cpu().numpy() for k, v in p.items()})
    assert losses[-1] / losses[0] < 1e-2
    for k, v in true.items():
        assert float((p[k].detach() - v).abs().max()) < 0.02, k

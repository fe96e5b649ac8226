"""GPU: the exact-fp32 conv block kernels (K5/K6) on their raw entry points, held to the independent fp64 references of
tests/helpers/f32block_refs64.py -- mx_conv_pack_weights, mx_plane_stats (the sweep), mx_plane_sum, mx_conv_block_fwd,
mx_conv_block_dgrad, mx_conv_block_wgrad (conv2d.hip, wgrad.hip, norm.hip, optim.hip).  tests/test_gpu_conv_units.py stays the
chain test of the family.

Conventions of tests/helpers/gpu_harness.py: every output lives between two guard bands pre-filled with a NaN bit pattern that
must survive; the pad columns of every fp32 input (in, x, G) hold 1e30, those of amax 0 / 1 / 2 mixed; every launch has valid
arguments; every tolerance gate is ``worst ratio to its bound <= 1``.

* exact tests: integer problems on which every fp32 operation of the kernels is exact in any order (f32block_refs64's module
  text), so the results must equal the fp64 reference bit for bit; ties between the pooled rows are frequent, which pins "first
  max on ties"; tests/test_f32block_refs64.py::test_defects_are_seen shows what each comparison catches;
* rounding tests: Gate A (derived, per element) and Gate B (the project's parity numbers, against fp64) of the same module
  text; the argmax is held to the reference's outside a band of 1e-5 max |z| that holds at most 1e-3 of the elements.
"""
import numpy as np
import pytest
import torch

from tests.helpers import f32block_refs64 as F
from tests.helpers.gpu_harness import ARG, UNSUPPORTED, Out, bits, call, dv, f32, f64, ratio, status

pytestmark = pytest.mark.gpu
P = F.PITCH
_CASES = [(s, T) for s in F.EXACT_SHAPES_DENSE for T in F.DILATIONS]
_ids = lambda c: "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c)
# what the shapes are chosen for: every halo row outside (H = 2), Wv below the halo (1, 17), the last vector partly / fully
# valid (351, 352), one clip
assert {2, 16} <= {H for _, H, _ in F.EXACT_SHAPES_DENSE} and {1, 17, 351, 352} <= {w for _, _, w in F.EXACT_SHAPES_DENSE}
assert any(B == 1 for B, _, _ in F.EXACT_SHAPES_DENSE)


def _mismatch(got, want):
    bad = np.argwhere(bits(got) != bits(want))
    return (bad.shape[0], bad[:4].tolist(), [float(got[tuple(k)]) for k in bad[:4]], [float(want[tuple(k)]) for k in bad[:4]])


def _opt(dev, a):
    return None if a is None else dv(dev, a)


# ==== layouts ==========================================================================================================================
@pytest.mark.parametrize("Cout,Cin", [(64, 64), (64, 2), (5, 3)])
def test_pack_weights(dev, Cout, Cin):
    g = np.random.default_rng(Cout * 100 + Cin)
    W = g.standard_normal((Cout, Cin, 5, 13)).astype(f32)
    for flip in (0, 1):
        o = Out(dev, W.size)
        call("mx_conv_pack_weights", dv(dev, W), Cout, Cin, flip, o)
        assert o.guards_intact() and o.untouched() == 0
        assert np.array_equal(bits(o.read()), bits(F.pack_weights(W, flip).ravel())), flip


# ==== statistics and plane sums ========================================================================================================
_ST_CASES = [(H, Wv) for H in (1, 2, 3, 4, 16) for Wv in (1, 17, 345, 352)]


@pytest.mark.parametrize("H,Wv", _ST_CASES)
def test_plane_stats_sweep(dev, H, Wv):
    """mean and rstd of PReLU(x) (or of x) over the H x Wv valid region against block1_refs64.plane_stats in fp64, within
    f32block_refs64.stats_ref's bound.  The kernel's arithmetic, from which the bound is derived there: the slope product
    rounded to fp32 (2^-24 of each term on the slope branch), fp64 sums of the n = H Wv terms and of their squares
    (gamma64(n) of the sums of magnitudes), var = ss / n - mean^2 (the cancellation: gamma64(n + 6) (mean t^2 + mean^2), which at
    |mean| / std = 1e3 is 1e6 times the variance's own rounding), rstd = 1 / sqrt(var + eps) (d rstd <= d var / 2 (var + eps -
    d var)^1.5), one rounding of each result to fp32.  Plane 0 is exactly constant: rstd = 1 / sqrt(eps) to that bound; planes 1
    and 2 have mean / std = +-1e3.  C = 1, 3, 64 with and without a slope: the slope of plane p is slope[p % C]."""
    B = 2
    worst = 0.0
    for C in (1, 3, 64):
        for with_slope in (True, False):
            x, slope = F.stats_problem(B, C, H, Wv, with_slope)
            ref, bound = F.stats_ref(x, slope, Wv)
            o = Out(dev, B * C * 2)
            call("mx_plane_stats", dv(dev, x), _opt(dev, slope), B, C, H, Wv, float(F.EPS), o)
            got = o.read().reshape(B, C, 2)
            assert o.guards_intact()
            r = ratio(got, ref, bound)
            worst = max(worst, r)
            assert r <= 1.0, (C, with_slope, r)
            assert ratio(got[0, 0, 1], 1.0 / np.sqrt(F.EPS), bound[0, 0, 1]) <= 1.0 and bound[0, 0, 1] < 1e-4 * ref[0, 0, 1]
    print(f"[measured] plane_stats H={H} Wv={Wv}: worst ratio to the derived bound {worst:.3f}")


@pytest.mark.parametrize("H,Wv", _ST_CASES)
def test_plane_sum(dev, H, Wv):
    """The fp64 sum of the valid region rounded once: 2^-24 of the sum plus gamma64(n) of the sum of magnitudes."""
    worst = 0.0
    for C in (1, 3, 64):
        x, _ = F.stats_problem(2, C, H, Wv, False)
        s, bound = F.sum_ref(x, Wv)
        o = Out(dev, 2 * C)
        call("mx_plane_sum", dv(dev, x), 2 * C, H, Wv, o)
        assert o.guards_intact()
        r = ratio(o.read().reshape(2, C), s, bound)
        worst = max(worst, r)
        assert r <= 1.0, (C, r)
    print(f"[measured] plane_sum H={H} Wv={Wv}: worst ratio to the bound {worst:.3f}")


# ==== exact on integers ================================================================================================================
def _run_fwd(dev, p, B, Cin, H, Wv, T):
    n = B * 64 * (H // 2) * P
    out, am = Out(dev, n), Out(dev, n, np.uint8)
    call("mx_conv_block_fwd", dv(dev, p["x"]), dv(dev, p["stats"]), _opt(dev, p["slope"]), dv(dev, F.pack_weights(p["W"], 0)),
         dv(dev, p["bias"]), B, Cin, H, Wv, T, 1 if p["slope"] is None else 0, out, am)
    assert out.guards_intact() and am.guards_intact()
    got, gam = out.read().reshape(B, 64, H // 2, P), am.read().reshape(B, 64, H // 2, P)
    assert not bits(got[..., Wv:]).any()                                      # pad columns of out: zero words
    assert gam[..., Wv:].size == 0 or gam[..., Wv:].max() <= 1                # pad columns of out_amax: 0 or 1
    return got[..., :Wv], gam[..., :Wv]


@pytest.mark.parametrize("case", [c + (Cin,) for c in _CASES for Cin in (2, 64)] + [((3, 6, 40), 2, 4)], ids=_ids)
def test_fwd_exact_on_integers(dev, case):
    """Cin = 2 is the first layer (no slope), Cin = 64 and the one Cin = 4 case apply the PReLU on the fly.  out and out_amax
    equal the reference bit for bit; ties (the rows of the last clip are alike; channels 0, 16, .. tie at the image's edge too)
    keep the first row."""
    (B, H, Wv), T, Cin = case
    p, ref = F.exact_problem(B, H, Wv, Cin), F.exact_fwd(B, H, Wv, Cin, T)
    assert ref["ties"] > 0
    got, gam = _run_fwd(dev, p, B, Cin, H, Wv, T)
    assert np.array_equal(bits(got), bits(ref["out"])), _mismatch(got, ref["out"])
    assert np.array_equal(gam, ref["amax"]), np.argwhere(gam != ref["amax"])[:4].tolist()


def _run_dgrad(dev, gr, W, B, H, Wv, T):
    dx = Out(dev, B * 64 * H * P)
    call("mx_conv_block_dgrad", dv(dev, gr["G"]), dv(dev, gr["amax"], np.uint8), dv(dev, F.pack_weights(W, 1)), B, H, Wv, T, dx)
    got = dx.read().reshape(B, 64, H, P)
    assert dx.guards_intact() and not bits(got[..., Wv:]).any()               # pad columns of dxhat: zero words
    return got[..., :Wv]


@pytest.mark.parametrize("case", _CASES, ids=_ids)
def test_dgrad_exact_on_integers(dev, case):
    (B, H, Wv), T = case
    p, ref = F.exact_problem(B, H, Wv, 64), F.exact_dgrad(B, H, Wv, T)
    got = _run_dgrad(dev, p, p["W"], B, H, Wv, T)
    assert np.array_equal(bits(got), bits(ref["dx"])), _mismatch(got, ref["dx"])


def _run_wgrad(dev, p, gr, B, Cin, H, Wv, T, rps):
    """-> (dW (64, Cin, 5, 13), part (slabs, 5, 13, 64, Cin)); no word of the workspace keeps the sentinel."""
    n_slabs = -(-B * H // rps)
    part, dW = Out(dev, n_slabs * F.TAPS * 64 * Cin), Out(dev, 64 * Cin * F.TAPS)
    call("mx_conv_block_wgrad", dv(dev, gr["G"]), dv(dev, gr["amax"], np.uint8), dv(dev, p["x"]), dv(dev, p["stats"]),
         _opt(dev, p["slope"]), B, Cin, H, Wv, T, rps, part, dW)
    assert part.guards_intact() and dW.guards_intact()
    assert part.untouched() == 0 and dW.untouched() == 0, (rps, part.untouched())
    return dW.read().reshape(64, Cin, 5, 13), part.read().reshape(n_slabs, 5, 13, 64, Cin)


@pytest.mark.parametrize("case", [c + (Cin,) for c in _CASES for Cin in (2, 64)], ids=_ids)
def test_wgrad_exact_on_integers(dev, case):
    """Cin = 64, and Cin = 2 with slope = NULL; one row per slab, three (at H = 4: a slab across the clip boundary), one slab
    for the whole batch, and a slab longer than the batch.  dW is bit-exact; the workspace equals the per-slab reference bit for
    bit (up to 8 slabs; its fp64 sum over the slabs gives dW for every count); at H = 2 with one row per slab the slab of row
    h = 0 has no valid row for kh = 0, 1 and 4, the slab of row h = 1 none for kh = 0, 3 and 4: those partials are zeros."""
    (B, H, Wv), T, Cin = case
    p, ref = F.exact_problem(B, H, Wv, Cin), F.exact_wgrad(B, H, Wv, Cin, T)
    for rps in (1, 3, B * H, B * H + 5):
        got, part = _run_wgrad(dev, p, p, B, Cin, H, Wv, T, rps)
        assert np.array_equal(bits(got), bits(ref["dW"])), (rps,) + _mismatch(got, ref["dW"])
        assert np.array_equal(part.astype(f64).sum(0).transpose(2, 3, 0, 1), ref["dW"].astype(f64)), rps
        if part.shape[0] == 1:
            assert np.array_equal(bits(part[0].transpose(2, 3, 0, 1)), bits(ref["dW"])), rps
        elif part.shape[0] <= 8:
            want = F.exact_wgrad_parts(B, H, Wv, Cin, T, rps)
            assert np.array_equal(bits(part), bits(want)), (rps,) + _mismatch(part, want)
        if H == 2 and rps == 1:
            for s in range(part.shape[0]):
                assert not bits(part[s, [0, 1, 4] if s % 2 == 0 else [0, 3, 4]]).any(), s


@pytest.mark.parametrize("Cin", [2, 64])
def test_wgrad_of_a_zero_gradient(dev, Cin):
    """G == 0 in the valid columns (1e30 in its pad columns): dW == 0."""
    B, H, Wv, T = 2, 4, 345, 1
    p = F.exact_problem(B, H, Wv, Cin)
    gr = dict(G=F.planes(np.zeros((B, 64, H // 2, Wv), f32), Wv), amax=p["amax"])
    got, part = _run_wgrad(dev, p, gr, B, Cin, H, Wv, T, 3)
    assert not got.any() and not part.any()


# ==== rounding on floats ===============================================================================================================
_RCASES = [(s, T) for s in F.ROUNDING_SHAPES for T in F.DILATIONS]


@pytest.mark.parametrize("case", [c + (Cin,) for c in _RCASES for Cin in (2, 64)] + [((3, 6, 40), 2, 4)], ids=_ids)
def test_fwd_rounding(dev, case):
    """Gaussian inputs with the GIVEN fp32 statistics against the fp64 evaluation of the same inputs: Gate A, Gate B (5e-6 of
    max |out|), and the argmax equal to the reference's wherever the fp64 rows differ by more than 1e-5 max |z| (at most 1e-3 of
    the elements lie inside that band: asserted from the reference alone in f32block_refs64.float_fwd)."""
    (B, H, Wv), T, Cin = case
    p, ref = F.float_problem(B, H, Wv, Cin), F.float_fwd(B, H, Wv, Cin, T)
    assert 1.0 - ref["decided"].mean() <= F.BAND_SHARE
    got, gam = _run_fwd(dev, p, B, Cin, H, Wv, T)
    a, b = ratio(got, ref["out"], ref["bound"]), ratio(got, ref["out"], F.gate_b("fwd", ref["out"]))
    wrong = int((gam != ref["amax"])[ref["decided"]].sum())
    print(f"[measured] f32 fwd {B}x{H}x{Wv} T={T} Cin={Cin}: gate A {a:.4f}, gate B {b:.4f} (err / max = {b * F.GATE_B['fwd']:.2e}), "
          f"undecided {int((~ref['decided']).sum())}, argmax differs inside the band {int((gam != ref['amax']).sum()) - wrong}")
    assert a <= 1.0
    assert b <= 1.0
    assert wrong == 0


@pytest.mark.parametrize("case", _RCASES, ids=_ids)
def test_dgrad_rounding(dev, case):
    """Gaussian, heavy-tailed (2^-k, k = 0..14) and mostly-zero (seven planes of eight exactly 0) pooled gradients: Gate A and
    Gate B (1e-5 of max |dxhat|)."""
    (B, H, Wv), T = case
    W = F.float_problem(B, H, Wv, 64)["W"]
    for kind in F.GRAD_KINDS:
        ref = F.float_dgrad(B, H, Wv, T, kind)
        got = _run_dgrad(dev, F.float_grads(B, H, Wv, kind), W, B, H, Wv, T)
        a, b = ratio(got, ref["dx"], ref["bound"]), ratio(got, ref["dx"], F.gate_b("dgrad", ref["dx"]))
        print(f"[measured] f32 dgrad {B}x{H}x{Wv} T={T} {kind}: gate A {a:.4f}, gate B {b:.4f} (err / max = {b * F.GATE_B['dgrad']:.2e})")
        assert a <= 1.0, kind
        assert b <= 1.0, kind


@pytest.mark.parametrize("case", [c + (Cin,) for c in _RCASES for Cin in (2, 64)], ids=_ids)
def test_wgrad_rounding(dev, case):
    """The same gradients through the weight gradient, three rows per slab and one slab for the whole batch: Gate A and Gate B
    (1e-5 of max |dW|)."""
    (B, H, Wv), T, Cin = case
    p = F.float_problem(B, H, Wv, Cin)
    for kind in F.GRAD_KINDS:
        ref = F.float_wgrad(B, H, Wv, Cin, T, kind)
        for rps in (3, B * H):
            got, _ = _run_wgrad(dev, p, F.float_grads(B, H, Wv, kind), B, Cin, H, Wv, T, rps)
            a, b = ratio(got, ref["dW"], ref["bound"]), ratio(got, ref["dW"], F.gate_b("wgrad", ref["dW"]))
            print(f"[measured] f32 wgrad {B}x{H}x{Wv} T={T} Cin={Cin} {kind} rps={rps}: gate A {a:.4f}, gate B {b:.4f} "
                  f"(err / max = {b * F.GATE_B['wgrad']:.2e})")
            assert a <= 1.0, (kind, rps)
            assert b <= 1.0, (kind, rps)


# ==== documented statuses ==============================================================================================================
def test_documented_statuses_without_a_launch(dev):
    """Every refusal happens before a launch: the outputs keep their sentinel words.  (The buffers are large enough for the
    base arguments: B = 1, H = 2, Wv = 8, Cin = 2.)"""
    z = torch.zeros(1 << 19, device=dev)
    outs = []

    def out():
        outs.append(Out(dev, 1 << 16))
        return outs[-1]

    base = dict(B=1, H=2, Wv=8, T=1, Cin=2)

    def fwd(**k):
        a = dict(dict(base, x=z, stats=z, slope=z, wt=z, bias=z, first=0, out=out(), amax=out()), **k)
        return status("mx_conv_block_fwd", a["x"], a["stats"], a["slope"], a["wt"], a["bias"], a["B"], a["Cin"], a["H"], a["Wv"], a["T"],
                      a["first"], a["out"], a["amax"])

    def dgrad(**k):
        a = dict(dict(base, G=z, amax=z, wt=z, out=out()), **k)
        return status("mx_conv_block_dgrad", a["G"], a["amax"], a["wt"], a["B"], a["H"], a["Wv"], a["T"], a["out"])

    def wgrad(**k):
        a = dict(dict(base, G=z, amax=z, x=z, stats=z, slope=None, rps=1, part=out(), dW=out()), **k)
        return status("mx_conv_block_wgrad", a["G"], a["amax"], a["x"], a["stats"], a["slope"], a["B"], a["Cin"], a["H"], a["Wv"], a["T"],
                      a["rps"], a["part"], a["dW"])

    # MX_ERR_ARG: every pointer the entry points check, a later layer without its slope, no rows in a slab
    for entry, names in ((fwd, ("x", "stats", "wt", "bias", "out", "amax")), (dgrad, ("G", "amax", "wt", "out")),
                         (wgrad, ("G", "amax", "x", "stats", "part", "dW"))):
        for name in names:
            assert entry(**{name: None}) == ARG, (entry.__name__, name)
    assert fwd(slope=None) == ARG and fwd(slope=None, first=1, T=3) == UNSUPPORTED      # (the first layer needs no slope)
    assert wgrad(rps=0) == ARG and wgrad(rps=-1) == ARG
    assert status("mx_conv_pack_weights", None, 64, 2, 0, out()) == ARG and status("mx_conv_pack_weights", z, 64, 2, 0, None) == ARG
    assert status("mx_plane_stats", None, None, 1, 2, 2, 8, 1e-5, out()) == ARG and status("mx_plane_stats", z, None, 1, 2, 2, 8, 1e-5, None) == ARG
    assert status("mx_plane_sum", None, 2, 2, 8, out()) == ARG and status("mx_plane_sum", z, 2, 2, 8, None) == ARG
    # MX_ERR_UNSUPPORTED: sizes
    for entry in (fwd, dgrad, wgrad):
        for k in (dict(H=3), dict(H=1), dict(H=0), dict(Wv=0), dict(Wv=353), dict(T=3)):
            assert entry(**k) == UNSUPPORTED, (entry.__name__, k)
    assert fwd(B=65536) == UNSUPPORTED and dgrad(B=65536) == UNSUPPORTED
    for cin in (0, 1, 3):
        assert fwd(Cin=cin) == UNSUPPORTED, cin
    for cin in (1, 3, 4, 32):
        assert wgrad(Cin=cin, slope=z) == UNSUPPORTED, cin
    assert wgrad(Cin=64, slope=None) == UNSUPPORTED
    assert wgrad(B=65536) == UNSUPPORTED and wgrad(B=16384, H=4) == UNSUPPORTED      # 131072 and 65536 slabs of one row
    for o in outs:
        assert o.guards_intact() and o.untouched() == o.words

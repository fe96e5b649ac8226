"""GPU: the rate contour (K25: csrc/rate_track.hip, ``rate_track.fit_rate_track``) against its definition in numpy,
tests/helpers/rate_track64.py, at the smallest shapes at which the kernels can go wrong.

Gates (none of them measured on the kernel):
NODE.  A node is R / Syy of one candidate, K23's three sums.  tests/test_gpu_lfo_fit.py derives what the device's cosine can move:
|dt_i| <= 2.5 x 2^-23 = 3e-7 a point, so sqrt(R) moves by at most a sqrt(n) 3e-7 and, with a sqrt(n) std(t) <= sqrt(Syy),
sqrt(R / Syy) by e = 3e-7 / std(t).  That file evaluates the bound at its winners (resid <= 1.1e-2, std(t) >= 0.28); a node table
holds EVERY candidate, so the bound is taken per candidate with its own node value and its own std(t) over the slice:
|d node| <= 2 sqrt(node) e + e^2, plus 1e-12 for the fp64 sums (Stt - St^2 / n in the kernel, centred sums in the helper).
PATH.  ``grid_k``, ``grid_j``, ``shape`` equal the helper's; where a path differs, its price on the HELPER's node table
(``path_cost``) may exceed the helper's optimum by at most 1e-6, the project's excess gate for a choice between candidates, and
at most 2 % of the (row, slice) pairs of ALL the module's cases together may differ (test_the_cap_on_differing_paths, on a
module-scoped run of every case: of 46 pairs, none; every differing case is printed).  The CPU side of that
cap, the helper against itself on node tables moved by an ulp, is tests/test_rate_track64.py::test_an_ulp_on_the_nodes.
SLICES.  K18's gates (tests/test_gpu_lfo_fit.py): the helper's evaluation of the kernel's (shape, rate, phase) may exceed the
helper's own refined minimum from the same grid candidate by at most 1e-6 in R / Syy (the rows are clean or carry 0.01 noise:
resid <= 1.1e-2, the gate's premise, asserted; the row with a constant span is no LFO where the span cuts a slice, and on that
row alone the same derivation is evaluated at the slice's own resid and std(t)); amp, offset and resid within 2^-23 relative (resid: absolute, as there) of the
helper's fp64 objective on the template the device writes at the kernel's candidate.
S = 1 against ``fit_lfo``, second launches and the poisoned fills: bit for bit.

FAIL WITHOUT THE FEATURE: every test here (the entry points and ``rate_track`` do not exist).
Measured on the MI355X: profiles/r27/README.md."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests.helpers import lfo_fit64 as h
from tests.helpers import rate_track64 as r
from tests.helpers.rate_track_cases import CASES, SIX, case

pytestmark = pytest.mark.gpu
GATE = 1e-6
EPS = 2.0 ** -23
COS_ERR = 3e-7
PREMISE = 1.1e-2

def template_std(W, sr, sh, window, J):
    """std(t) of every coarse candidate of a W-point slice, (C,)"""
    f_min, f_max, srf, df, K = r.grid(W, sr, window[0], window[1], 4)
    f, p = h._decode(np.arange(K * J), J, 0, f_min, df, 0.0, h.TWO_PI / J, f_min, f_max)
    f32, ph32 = h.candidate(sh, f, p, W, srf)
    return h.template(W, srf, sh, f32, ph32).astype(np.float64).std(axis=1)


def raw_rate_track(dev, y_dev, stride, B, n, W, sr, starts, window, mask, J, D, L=4, rate_weight=0.002, phase_weight=1.0, pad=3):
    """The three enqueues on buffers of exactly the planned sizes, each with sentinels behind what the call owns: (outputs by
    name, the node table (B, 7, S, C) with NaN where nobody wrote)."""
    from mod_extraction_amd import _hip
    S = len(starts)
    sizes = (ctypes.c_int64 * 3)()
    a = ctypes.addressof(sizes)
    _hip.call("mx_rate_track_plan", B, n, sr, S, W, window[0], window[1], mask, 4, J, L, D, a, a + 8, a + 16)
    K = sizes[0]
    assert K == r.grid(W, sr, window[0], window[1], 4)[4] and sizes[1] == 8 * B * 7 * S * K * J and sizes[2] % 16 == 0
    node = torch.full((sizes[1] // 8 + 8,), float("nan"), device=dev, dtype=torch.float64)
    ws = torch.full((sizes[2] + 64,), 0xA5, device=dev, dtype=torch.uint8)
    assert node.data_ptr() % 16 == 0 and ws.data_ptr() % 16 == 0
    st = torch.tensor(starts, dtype=torch.int64, device=dev)
    i32 = lambda *s: torch.full(s, -777, device=dev, dtype=torch.int32)
    f32 = lambda *s: torch.full(s, -777.0, device=dev, dtype=torch.float32)
    o = {"shape": i32(B + pad), "grid_k": i32(B + pad, S), "grid_j": i32(B + pad, S), "cost": f32(B + pad),
         "per_shape_cost": f32(B + pad, 7)}
    o.update({k: f32(B + pad, S) for k in ("rate_hz", "phase", "amp", "offset", "resid")})
    grid = (window[0], window[1], mask, 4, J)
    buf = (node.data_ptr(), sizes[1], ws.data_ptr(), sizes[2])
    s_ = _hip.stream()
    _hip.call("mx_rate_track_nodes", y_dev.data_ptr(), stride, B, n, sr, st.data_ptr(), S, W, *grid, *buf, s_)
    _hip.call("mx_rate_track_path", B, n, sr, st.data_ptr(), S, W, *grid, D, rate_weight, phase_weight, *buf,
              *[o[k].data_ptr() for k in ("shape", "grid_k", "grid_j", "cost", "per_shape_cost")], s_)
    _hip.call("mx_rate_track_refine", y_dev.data_ptr(), stride, B, n, sr, st.data_ptr(), S, W, *grid, L,
              *[o[k].data_ptr() for k in ("shape", "grid_k", "grid_j", "rate_hz", "phase", "amp", "offset", "resid")], buf[2],
              buf[3], s_)
    torch.cuda.synchronize()
    for k, v in o.items():
        assert bool((v[B:] == -777).all()), k                                 # nothing behind the rows is touched
    assert bool(torch.isnan(node[sizes[1] // 8:]).all()) and bool((ws[sizes[2]:] == 0xA5).all())
    return {k: v[:B].cpu().numpy() for k, v in o.items()}, node[:sizes[1] // 8].view(B, 7, S, K * J).cpu().numpy()


def wide_rows(dev, y):
    """The rows a stride of n + 1 apart, the first one float off a 16-byte boundary; read in place."""
    B, n = y.shape
    flat = torch.full((B * (n + 1) + 1,), float("nan"), device=dev)
    view = flat[1:].view(B, n + 1)[:, :n]
    view.copy_(torch.from_numpy(y).to(dev))
    assert view.data_ptr() % 16 == 4 and view.stride() == (n + 1, 1)
    return view


@pytest.fixture(scope="module")
def runs(dev):
    """{case: (outputs, node table)}: the kernels on EVERY case, once, so that what is counted over all cases does not depend on
    which tests are selected or in what order they run."""
    out = {}
    for name, (n, W, hop, sr, window, J, D, shapes, rows, const) in CASES.items():
        y, starts, _ = case(name)
        out[name] = raw_rate_track(dev, wide_rows(dev, y), n + 1, len(y), n, W, sr, starts, window, h.mask_of(shapes), J, D)
    return out


def differing(name, k):
    """[(row, slices that differ from the helper's path, slices)] of a case; another shape counts as every slice."""
    J = CASES[name][5]
    _, starts, ref = case(name)
    out = []
    for b in range(len(ref)):
        path = k["grid_k"][b].astype(np.int64) * J + k["grid_j"][b]
        out.append((b, int((path != ref[b]["path"]).sum()) if k["shape"][b] == ref[b]["shape"] else len(starts), len(starts)))
    return out


def test_the_cap_on_differing_paths(runs):
    """At most 2 % of ALL (row, slice) pairs of the module's cases may differ from the helper's path: of 46, none."""
    counts = [c for name in CASES for c in differing(name, runs[name][0])]
    pairs, diff = sum(c[2] for c in counts), sum(c[1] for c in counts)
    print(f"paths: {diff} of {pairs} (row, slice) pairs differ from the helper's")
    assert pairs == 46 and diff <= 0.02 * pairs


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_against_the_helper(dev, runs, name):
    from mod_extraction_amd import modulations as M
    n, W, hop, sr, window, J, D, shapes, rows, const = CASES[name]
    y, starts, ref = case(name)
    B, S = len(y), len(starts)
    k, node = runs[name]
    per_row = dict((b, d) for b, d, _ in differing(name, k))
    allowed = [h.SHAPE_IDS[s] for s in shapes]
    std_t = {sh: template_std(W, sr, sh, window, J) for sh in allowed}
    whole = [const is None or const[0] != b for b in range(B)]               # rows that are an LFO throughout
    worst_node = worst = 0.0
    for b in range(B):
        # nodes
        for sh in range(7):
            if sh not in allowed:
                assert bool(np.isnan(node[b, sh]).all())                      # a masked shape's cells are written by nobody
                continue
            want = ref[b]["nodes"][sh]
            e = COS_ERR / std_t[sh][None, :]
            tol = 2.0 * np.sqrt(want) * e + e * e + 1e-12
            ratio = float((np.abs(node[b, sh] - want) / tol).max())
            worst_node = max(worst_node, ratio)
            assert ratio <= 1.0, (b, sh, ratio)
        # the path
        path = k["grid_k"][b].astype(np.int64) * J + k["grid_j"][b]
        diff = per_row[b]
        args = (starts, ref[b]["sr"], ref[b]["fk"], J, D, 0.002, 1.0)
        if diff:
            sh = int(k["shape"][b])
            price = r.path_cost(ref[b]["nodes"][sh], path, sh, *args)
            print(f"{name} row {b}: {diff} of {S} slices differ; kernel {h.SHAPES[sh]} {path.tolist()} at {price:.9f} on the helper's "
                  f"nodes, helper {h.SHAPES[ref[b]['shape']]} {ref[b]['path'].tolist()} at {ref[b]['cost']:.9f}")
            tol = GATE
            assert price - ref[b]["cost"] <= tol, (b, price, ref[b]["cost"])
        if not diff:                                                          # the same path: its nodes' bounds add up
            e = COS_ERR / std_t[ref[b]["shape"]][path]
            along = ref[b]["nodes"][ref[b]["shape"]][np.arange(S), path]
            tol = float((2.0 * np.sqrt(along) * e + e * e + 1e-12).sum()) + 2.0 ** -23 * ref[b]["cost"]
            assert abs(float(k["cost"][b]) - ref[b]["cost"]) <= tol, (b, float(k["cost"][b]), ref[b]["cost"], tol)
        assert [bool(np.isfinite(v)) for v in k["per_shape_cost"][b]] == [s in allowed for s in range(7)]
        assert k["per_shape_cost"][b][k["shape"][b]] == k["cost"][b]
        # the slices: K18's gates at the kernel's own grid candidate
        sh = int(k["shape"][b])
        t_dev = M.make_mod_signals(W, sr, torch.from_numpy(k["rate_hz"][b]).to(dev), torch.from_numpy(k["phase"][b]).to(dev),
                                   torch.full((S,), sh, dtype=torch.int32, device=dev)).cpu().numpy()
        for s in range(S):
            ys = y[b, starts[s]:starts[s] + W]
            mine = r.refine_slice(ys, sr, sh, window[0], window[1], 4, J, 4, int(path[s]))
            got = {q: float(k[q][b, s]) for q in ("rate_hz", "phase", "amp", "offset", "resid")}
            if h.row_stats(ys)[2] == 0.0:                                     # a constant slice keeps the path's candidate
                assert got == {"rate_hz": float(mine["rate_hz"]), "phase": float(mine["phase"]), "amp": 0.0,
                               "offset": float(np.float32(mine["offset"])), "resid": 0.0}, (b, s, got)
                continue
            if whole[b]:
                premise = mine["resid"]
                assert premise <= PREMISE, (b, s, premise)
            excess = h.eval_at(ys, sr, sh, got["rate_hz"], got["phase"])["resid"] - mine["resid"]
            o = h.objective(ys, t_dev[s])
            at = {"a": float(o["a"][0]), "b": float(o["b"][0]), "resid": float(o["R"][0] / o["Syy"])}
            d = (abs(got["amp"] - at["a"]) / abs(at["a"]), abs(got["offset"] - at["b"]) / abs(at["b"]), abs(got["resid"] - at["resid"]))
            worst = max(worst, *d)
            tol = GATE
            if not whole[b]:
                # GATE's derivation at this slice's own resid and std(t), only where the premise is not given (a slice cut by
                # the constant span is no LFO): one swap costs 2 sqrt(resid) e + e^2 a candidate, twice that for the pair
                e = COS_ERR / float(t_dev[s].astype(np.float64).std())
                tol = max(GATE, 2.0 * (2.0 * math.sqrt(mine["resid"]) * e + e * e))
            assert excess <= tol, (b, s, excess)
            tol = EPS
            assert max(d) <= tol, (b, s, d)
            assert 0.0 <= got["phase"] < 2.0 * math.pi and got["amp"] >= 0.0
    print(f"{name}: worst node error / its bound {worst_node:.3f}; worst amp / offset / resid error {worst:.3e}; "
          f"{sum(per_row.values())} of {B * S} (row, slice) pairs differ from the helper's path")


@pytest.mark.parametrize("shapes", [("tri",), SIX])
def test_one_slice_is_fit_lfo(dev, shapes):
    """S = 1: the outputs of ``mx_lfo_fit`` on the slice, bit for bit (K J = 2016 > 512: K18 sums in ascending i too; clean
    rows, on which the coarse grid and the refined fit pick the same shape)."""
    from mod_extraction_amd import modulations as M, rate_track as R
    rows = [("tri", 1.13, 2.0), ("cos", 0.83, 1.0), ("rect_cos", 1.61, 2.5)]
    y = np.stack([h.make_row(345, 172.5, s if len(shapes) > 1 else "tri", f, p) for s, f, p in rows])
    yd = torch.from_numpy(y).to(dev)
    rt = R.fit_rate_track(yd, 172.5, 345, shapes=shapes)
    k18 = M.fit_lfo(yd, 172.5, shapes=shapes, per_shape=True)
    assert rt.starts.tolist() == [0] and rt.rate_hz.shape == (3, 1)
    assert torch.equal(rt.shape, k18.shape)
    for q in ("rate_hz", "phase", "amp", "offset", "resid"):
        assert torch.equal(getattr(rt, q)[:, 0], getattr(k18, q)), q


def test_plumbing_and_second_launch(dev):
    from mod_extraction_amd import rate_track as R
    n, W, hop, sr, window, J, D, shapes, rows, const = CASES["w16"]
    y, starts, ref = case("w16")
    kw = dict(hop_points=hop, rate_hz=window, shapes=shapes, n_phases=J, max_rate_step=D)
    yd = torch.from_numpy(y).to(dev)
    a, b = R.fit_rate_track(yd, sr, W, **kw), R.fit_rate_track(yd, sr, W, **kw)
    tensors = lambda rt: [v for v in rt if isinstance(v, torch.Tensor)]
    assert all(torch.equal(p, q) for p, q in zip(tensors(a), tensors(b)))    # two launches: the same bits
    assert all(torch.equal(p, q) for p, q in zip(tensors(a), tensors(R.fit_rate_track(wide_rows(dev, y), sr, W, **kw))))
    one = R.fit_rate_track(yd[1], sr, W, **kw)                                # a 1-d row
    assert torch.equal(one.rate_hz[0], a.rate_hz[1]) and torch.equal(one.grid_k[0], a.grid_k[1])
    assert a.starts.tolist() == starts and (a.slice_points, a.n_points, a.sr) == (W, n, sr)
    assert a.shape.tolist() == [ref[i]["shape"] for i in range(3)]
    times, rates = R.rate_at(a)
    assert times.tolist() == [(s + 0.5 * (W - 1)) / sr for s in starts] and rates is a.rate_hz
    # the stitched template: S = 1 is the slice's template itself
    s1 = R.fit_rate_track(yd[0, :W], sr, W, **kw)
    from mod_extraction_amd import modulations as M
    fit = M.LFOFit(s1.shape, s1.rate_hz[0], s1.phase[0], s1.amp[0], s1.offset[0], s1.resid[0])
    assert torch.equal(R.synth_from_rate_track(s1), M.synth_from_fit(fit, W, sr)[0])


def test_poisoned_allocations(dev):
    """The node table, the workspace and every output come from ``torch.empty``: the 0 / 0.5 / NaN fills change no bit.  A
    constant slice and masked shapes are in the case: their cells are written by nobody and read by nobody."""
    from mod_extraction_amd import rate_track as R
    from tests.test_gpu_uninit_independence import run_patterns
    n, W, hop, sr, window, J, D, shapes, rows, const = CASES["w16"]
    yd = torch.from_numpy(case("w16")[0]).to(dev)

    def run():
        rt = R.fit_rate_track(yd, sr, W, hop_points=hop, rate_hz=window, shapes=("cos", "tri", "saw"), n_phases=J, max_rate_step=2)
        out = {k: v for k, v in rt._asdict().items() if isinstance(v, torch.Tensor) and k != "per_shape_cost"}
        out["per_shape_cost_allowed"] = rt.per_shape_cost[:, [0, 3, 4]]
        out["stitched"] = R.synth_from_rate_track(rt, 1)
        return out

    run_patterns(run, {"rate_track:fit_rate_track"})

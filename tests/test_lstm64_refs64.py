"""CPU: the fp64 references of tests/helpers/lstm64_refs64.py against torch autograd in float64 through
oracle.models.LSTMEffectModel (1e-12 relative), a plain fp32 emulation of the same formulae against every bound that
tests/test_gpu_lstm64_units.py applies to the kernels of csrc/lstm.hip (if plain fp32 arithmetic cannot meet a bound, the bound
is wrong, not the kernel), and that emulation with one seeded defect at a time against the same gates (a defect no gate sees
means the GPU tests have no teeth there)."""
import numpy as np
import pytest
import torch

from tests.helpers import general_refs64 as G
from tests.helpers import lstm64_refs64 as L

f32, f64 = np.float32, np.float64
KINDS = ("default", "hot", "contractive")


def rel(got, ref):
    ref = np.asarray(ref, f64)
    return float(np.abs(np.asarray(got, f64) - ref).max() / max(float(np.abs(ref).max()), 1e-300))


def t64(a):
    return torch.from_numpy(np.array(a, f64))


# ==== references against torch ===================================================================================================
@pytest.mark.parametrize("mode", ["l1", "dy"])
@pytest.mark.parametrize("kind,B,T", [("default", 3, 33), ("hot", 1, 17), ("contractive", 3, 34), ("default", 1, 1)])
def test_agreement_with_autograd(kind, B, T, mode):
    """y, the state, every parameter gradient (summed over the clips, and clip by clip through the additivity of the loss),
    the dgate-derived dlfo, on the L1-fused path (ties y == wet included: |.|'(0) = 0 in torch too) and the dy path."""
    from oracle.models import LSTMEffectModel
    p = L.problem(kind, B, T)
    m = LSTMEffectModel().double()
    with torch.no_grad():
        for name, key in (("lstm.weight_ih_l0", "w_ih"), ("lstm.weight_hh_l0", "w_hh"), ("lstm.bias_ih_l0", "b_ih"),
                          ("lstm.bias_hh_l0", "b_hh"), ("fc.weight", "fc_w"), ("fc.bias", "fc_b")):
            dict(m.named_parameters())[name].copy_(t64(p[key]).view_as(dict(m.named_parameters())[name]))
    assert [n for n, _ in m.named_parameters()] == ["lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0",
                                                    "fc.weight", "fc.bias"]
    m.hidden = (t64(p["h_in"])[None], t64(p["c_in"])[None])
    lat = t64(p["lfo"])[:, None].requires_grad_(True)
    y_t = m(t64(p["x"])[:, None], lat)[:, 0]
    wet = p["wet"].astype(f64).copy()
    wet[p["ties"]] = y_t.detach().numpy()[p["ties"]]                     # ties against the fp64 y itself
    q = dict(p, wet=wet)
    st, y, h1, c1 = L.fwd64(p)
    tol = 1e-12
    assert rel(y, y_t.detach().numpy()) <= tol
    assert rel(h1, m.hidden[0][0].detach().numpy()) <= tol and rel(c1, m.hidden[1][0].detach().numpy()) <= tol
    assert np.array_equal(st[:, -1, 320:], h1) and np.array_equal(st[:, -1, 256:320], c1)
    y = y_t.detach().numpy().copy()                                      # (agrees to 1e-12: the ties need the very same numbers)
    per_clip = p["loss_scale"] * (y_t - t64(wet)).abs().sum(1) if mode == "l1" else (y_t * t64(p["dy"])).sum(1)
    g = L.loss_grad(q, y, mode)
    if mode == "l1":
        assert not g[p["ties"]].any() and np.count_nonzero(g) == (~p["ties"]).sum()
    r = L._bptt(p, st, y, g)
    part, e_part, m_part = L._part(p, st, r["dgate"], r["e_dgate"], r["s_dgate"], r["dzy"], r["e_dzy"])
    params = list(m.parameters())
    for b in range(B):
        grads = torch.autograd.grad(per_clip[b], params + [lat], retain_graph=True)
        flat = np.concatenate([gr.numpy().ravel() for gr in grads[:-1]])
        assert flat.size == L.NPARAM
        for n, (lo, hi) in L.PARTS.items():
            assert rel(part[b, lo:hi], flat[lo:hi]) <= tol, (b, n)
        assert rel(L.dlfo64(p, r["dgate"])[0][b], grads[-1].numpy()[b, 0]) <= tol
    # the same BPTT from the general reference, and the local variants fed with the exact dgate reproduce it
    dhfc = r["dzy"][..., None] * p["fc_w"].astype(f64)
    assert rel(r["dgate"], G.lstmg_bwd(st.reshape(B, T, 6, 64), dhfc, p["w_hh"], p["c_in"])) <= tol
    assert rel(L.step_bwd(p, st, y, g, r["dgate"])["dgate"], r["dgate"]) <= tol
    assert rel(L.part_from_dgate(p, st, y, g, r["dgate"])[0], part) <= tol
    assert (np.abs(part) <= m_part * (1 + 1e-12)).all() and (np.abs(r["dgate"]) <= r["s_dgate"] * (1 + 1e-12)).all()


def test_step_fwd_is_the_recurrence():
    """step_fwd of the fp64 rows reproduces the fp64 rows; y_fwd the fp64 y."""
    p = L.problem("hot", 3, 17)
    st = p["stash64"]
    h_prev = np.concatenate([p["h_in"].astype(f64)[:, None], st[:, :-1, 320:]], 1)
    c_prev = np.concatenate([p["c_in"].astype(f64)[:, None], st[:, :-1, 256:320]], 1)
    v, _ = L.step_fwd(p, p["lfo"], p["x"], h_prev, c_prev)
    for q, n in enumerate("ifgoch"):
        assert rel(v[n], st[:, :, q * 64:(q + 1) * 64]) <= 1e-12, n
    assert rel(L.y_fwd(p, st[:, :, 320:], p["x"])[0], p["y64"]) <= 1e-12


def test_activation_bound_shape():
    """The derived bound at a few arguments, in units of u: 1 at sigmoid(0) (0.25 + 0.75), below 2.6 for every sigmoid
    argument up to 8 and growing with |x| only where the slope is not yet gone; tanh(0): 2 (0.25 + 0.75) = 2."""
    s = 1 + 2.0 ** -10
    assert abs(L.act_bound(0.0, 1) / L.U - 1.0 * s) < 1e-6 and abs(L.act_bound(0.0, 2) / L.U - 2.0 * s) < 1e-6
    x = np.linspace(-8, 8, 1001)
    assert (L.act_bound(x, 1) <= 2.6 * L.U).all() and (L.act_bound(x, 2) <= 4.1 * L.U).all()
    assert L.act_bound(4.0, 1) > 1.5 * L.U * G.sigmoid(4.0) * s and L.act_bound(-30.0, 1) < 1e-11 * L.U


# ==== the emulated fp32 arithmetic stays inside every bound ========================================================================
def _bwd_ratios(p, dgate, part, mode, local):
    """The gates of the backward GPU tests on (dgate, part): running bound (contractive) or local step + part_from_dgate."""
    g = L.loss_grad(p, p["y"], mode)
    if local:
        r = L.step_bwd(p, p["stash"], p["y"], g, dgate)
        ref, bnd = L.part_from_dgate(p, p["stash"], p["y"], g, dgate)
    else:
        r = L.running_ref(p["kind"], p["B"], p["T"], mode)
        ref, bnd = r["part"], r["e_part"]
    out = L.part_ratios(part, ref, bnd)
    out["dgate"] = L.ratio(dgate, r["dgate"], r["e_dgate"])
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", [1, 17, 48, 257])
def test_emulated_fp32_forward_within_bounds(kind, T):
    p = L.problem(kind, 3, T)
    out = L.fwd_gates(p, *L.emu_fwd(p, np.random.default_rng(T)))
    print("emu fwd", kind, T, {k: round(v, 3) for k, v in out.items()})
    tol = 1.0
    assert all(v <= tol for v in out.values()), out


@pytest.mark.parametrize("mode", ["l1", "dy"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", [1, 2, 33, 65])
def test_emulated_fp32_backward_within_bounds(kind, T, mode):
    """contractive: the running bound; default / hot: the local step from the emulation's own dgate."""
    p = L.problem(kind, 3, T)
    dgate, part = L.emu_bwd(p, p["stash"], p["y"], mode, np.random.default_rng(T))
    out = _bwd_ratios(p, dgate, part, mode, local=kind != "contractive")
    d, e = L.dlfo64(p, dgate)
    out["dlfo"] = L.ratio(L._seqdot(dgate, p["w_ih"][:, 0]), d, e)
    print("emu bwd", kind, T, mode, {k: round(v, 3) for k, v in out.items()})
    tol = 1.0
    assert all(v <= tol for v in out.values()), out
    if mode == "l1":                                                    # ties contribute exactly zero
        assert not L._bptt(p, p["stash"], p["y"], L.loss_grad(p, p["y"], "l1"))["dzy"][p["ties"]].any()


def test_contractive_set_keeps_the_running_bound_sharp():
    """bwd_running asserts bound <= 2^-10 of the magnitude sum per element; the default set must FAIL that condition at a
    length where the contractive one holds it (else the condition tests nothing)."""
    for T in (33, 129):
        L.running_ref("contractive", 3, T, "l1")
    p = L.problem("default", 1, 129)
    with pytest.raises(AssertionError):
        L.bwd_running(p, p["stash"], p["y"], L.loss_grad(p, p["y"], "dy"))


# ==== seeded defects ==============================================================================================================
_FWD_CASES = {"stash_early": ("default", 32), "swap_in": ("default", 17), "no_bhh": ("default", 17), "c_restart": ("default", 272),
              "act_err": ("hot", 48)}
_BWD_CASES = {"drop_dg1_h0": 33, "dg0_h0": 34, "skip_last_slab": 65, "f_carry": 34, "tanh_prev_row": 34, "no_bias_hh": 5,
              "sign0": 34, "df0_zero_cinit": 34}


def test_defects_are_seen():
    """Every seeded defect pushes the worst ratio of its gate above 4 (the clean emulation stays <= 1 on the same problem)."""
    margin = 4.0
    assert set(_FWD_CASES) == set(L.FWD_DEFECTS) and set(_BWD_CASES) == set(L.BWD_DEFECTS)
    for defect, (kind, T) in _FWD_CASES.items():
        p = L.problem(kind, 1, T)
        clean = L.fwd_gates(p, *L.emu_fwd(p, np.random.default_rng(1)))
        bad = L.fwd_gates(p, *L.emu_fwd(p, np.random.default_rng(1), defect))
        print("defect", defect, round(max(clean.values()), 3), {k: round(v, 2) for k, v in bad.items()})
        assert max(clean.values()) <= 1.0 and max(bad.values()) > margin, (defect, clean, bad)
    for defect, T in _BWD_CASES.items():
        p = L.problem("contractive", 3, T)
        # (sign0 exists on the L1 path only; the last sample of every clip is a tie, so the L1 path has nothing to lose at the
        #  last step: the skipped slab shows on the dy path)
        for mode in {"sign0": ("l1",), "skip_last_slab": ("dy",)}.get(defect, ("l1", "dy")):
            clean = _bwd_ratios(p, *L.emu_bwd(p, p["stash"], p["y"], mode, np.random.default_rng(1)), mode, False)
            bad = _bwd_ratios(p, *L.emu_bwd(p, p["stash"], p["y"], mode, np.random.default_rng(1), defect), mode, False)
            print("defect", defect, mode, round(max(clean.values()), 3), {k: round(v, 2) for k, v in bad.items()})
            assert max(clean.values()) <= 1.0 and max(bad.values()) > margin, (defect, mode, clean, bad)
    # the local gates of the default / hot sets see the defects of the recurrence itself too
    p = L.problem("default", 3, 33)
    for defect in ("f_carry", "tanh_prev_row", "df0_zero_cinit", "drop_dg1_h0", "dg0_h0"):
        bad = _bwd_ratios(p, *L.emu_bwd(p, p["stash"], p["y"], "dy", np.random.default_rng(1), defect), "dy", True)
        assert max(bad.values()) > margin, (defect, bad)

"""GPU: the LSTM-64 effect-model kernels of csrc/lstm.hip on their raw entry points -- mx_lstm_fwd, mx_lstm_bwd_l1, mx_lstm_bwd,
mx_lstm_bwd_dgate, mx_lstm_dlfo (and mx_reduce_rows on their gradient rows) -- held to the independent fp64 references and the
per-element bounds of tests/helpers/lstm64_refs64.py.  tests/test_gpu_lstm.py, test_gpu_edges.py and test_gpu_unfrozen.py stay
the model-level tests of the family.

Conventions of tests/test_gpu_midblock_units.py: every output is an ``Out`` between two guard bands pre-filled with a NaN bit
pattern that must survive; x, lfo, y, wet, dy (and the y / dlfo outputs) are rows of a larger buffer with a stride above T, every
row starting at an ODD float offset (4-byte aligned only), the floats between the rows holding 1e30 (inputs) or the sentinel
(outputs); B in {1, 3}; every derived gate is ``worst ratio to its bound <= tol`` with tol = 1.0.  u = 2^-23.

* forward: nothing is compared across steps -- every stash row against one fp64 step from the previous DEVICE row, y_t against
  the device's own h_t -- so the bound is as tight at step 527 as at step 0 and a fault at step t is reported at step t;
* backward, contractive weights (w_hh in +-1/32): the whole BPTT against fp64 with a running bound that the helper keeps within
  2^-10 of every element's magnitude sum; a zero bound (ties y == wet, where nothing may arrive) demands exact equality;
* backward, weights on the product scale: dgate[t] against one fp64 step from the device's dgate[t + 1], part against fp64 sums
  of the device's dgate; the training kernel (which leaves no dgate) against the yardstick of test_lstmg_recurrence;
* tests/test_lstm64_refs64.py::test_defects_are_seen shows on the CPU that these gates see thirteen seeded defects.

Measured on the MI355X, worst ratio of each derived gate over all cases (tol = 1.0): forward i 0.13, f 0.12, g 0.21, o 0.13,
c 0.07, h 0.14, y 0.02; contractive part 0.32 (w_hh), dgate 0.51; local dgate 0.54, part 0.15; every exact gate exact.
"""
import numpy as np
import pytest
import torch

from tests.helpers import lstm64_refs64 as L
from tests.helpers.gpu_harness import ARG, POISON, SENT, U, UNSUPPORTED, Out, bits, call, dv, f32, f64, ratio, status

pytestmark = pytest.mark.gpu
H, NG, STASH, NPARAM = L.H, L.NG, L.STASH, L.NPARAM
WEIGHTS = ("w_ih", "w_hh", "b_ih", "b_hh", "fc_w", "fc_b")


def dvc(dev, a):
    """A problem's (read-only) array to the device."""
    return dv(dev, np.array(a, f32))


def _stride(T):
    return T + 6 - (T % 2)                         # even and above T: with the offset 1 every row starts at an odd float


class RowsIn:
    """(B, T) values as rows of a 1e30-filled buffer: row b at float 1 + b stride."""

    def __init__(self, dev, a):
        a = np.asarray(a, f32)
        B, T = a.shape
        self.stride = _stride(T)
        buf = np.full(1 + B * self.stride + 3, POISON, f32)
        for b in range(B):
            buf[1 + b * self.stride:1 + b * self.stride + T] = a[b]
        self.t = dv(dev, buf)

    def ptr(self):
        return self.t.data_ptr() + 4


class RowsOut:
    """The same layout as an output: the gaps between the rows are sentinel words that must survive."""

    def __init__(self, dev, B, T):
        self.B, self.T, self.stride = B, T, _stride(T)
        self.o = Out(dev, 1 + B * self.stride + 3)

    def ptr(self):
        return self.o.ptr() + 4

    def read(self):
        """(rows (B, T), everything outside the rows untouched)."""
        body = self.o.read()
        idx = 1 + np.arange(self.B)[:, None] * self.stride + np.arange(self.T)[None]
        gap = np.ones(body.size, bool)
        gap[idx.ravel()] = False
        return body[idx], bool((bits(body)[gap] == SENT).all()) and self.o.guards_intact()


def _weights(dev, p):
    return {n: dvc(dev, p[n]) for n in WEIGHTS}


def _fwd(dev, p, lo=0, hi=None, h_in=None, c_in=None, with_stash=True, alias=False):
    """mx_lstm_fwd on steps [lo, hi) of the problem from the state (h_in, c_in); every output checked for strays."""
    B = p["B"]
    hi = p["T"] if hi is None else hi
    n = hi - lo
    h_in = p["h_in"] if h_in is None else h_in
    c_in = p["c_in"] if c_in is None else c_in
    w = _weights(dev, p)
    x, lfo = RowsIn(dev, p["x"][:, lo:hi]), RowsIn(dev, p["lfo"][:, lo:hi])
    y = RowsOut(dev, B, n)
    stash = Out(dev, B * n * STASH) if with_stash else None
    if alias:
        h_o, c_o = Out(dev, B * H, init=np.array(h_in)), Out(dev, B * H, init=np.array(c_in))
        h_i, c_i = h_o, c_o
    else:
        h_o, c_o, h_i, c_i = Out(dev, B * H), Out(dev, B * H), dvc(dev, h_in), dvc(dev, c_in)
    call("mx_lstm_fwd", x.ptr(), x.stride, lfo.ptr(), lfo.stride, w["w_ih"], w["w_hh"], w["b_ih"], w["b_hh"], w["fc_w"], w["fc_b"],
         h_i, c_i, h_o, c_o, y.ptr(), y.stride, stash, B, n)
    yv, y_clean = y.read()
    assert y_clean and h_o.guards_intact() and c_o.guards_intact()
    assert h_o.untouched() == 0 and c_o.untouched() == 0
    out = dict(y=yv, h_out=h_o.read().reshape(B, H), c_out=c_o.read().reshape(B, H), stash=None)
    if with_stash:
        assert stash.guards_intact() and stash.untouched() == 0                      # no sentinel word left in the stash
        out["stash"] = stash.read().reshape(B, n, STASH)
    return out


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


# ==== forward =====================================================================================================================
FWD_T = [1, 2, 15, 16, 17, 48, 255, 256, 257, 272, 528]


@pytest.mark.parametrize("kind", ["default", "hot"])
@pytest.mark.parametrize("T", FWD_T)
def test_fwd_one_step_consistency(dev, kind, T):
    """16 | 48 | 256 | 272 | 528: unrolled groups of 16 (one group, three, a whole block, a block of exactly one group behind a
    full one, a third block); 1 | 2 | 15 | 17 | 255 | 257: the rolled loop (a partial group; one step behind a full block).
    Every stash row against step_fwd of the previous device row, y_t against the device's h_t, h_out / c_out bit-equal to the
    h / c planes of the last stash row."""
    for B in (1, 3):
        p = L.problem(kind, B, T)
        r = _fwd(dev, p)
        out = L.fwd_gates(p, r["stash"], r["y"], r["h_out"], r["c_out"])
        print("lstm64 fwd", kind, T, B, {k: round(v, 3) for k, v in out.items()})
        tol = 1.0
        assert out["i"] <= tol, (B, out)
        assert out["f"] <= tol, (B, out)
        assert out["g"] <= tol, (B, out)
        assert out["o"] <= tol, (B, out)
        assert out["c"] <= tol, (B, out)
        assert out["h"] <= tol, (B, out)
        assert out["y"] <= tol, (B, out)
        assert out["state"] == 0, B


@pytest.mark.parametrize("T", FWD_T)
def test_fwd_without_stash_and_aliased_state(dev, T):
    """stash = NULL selects the second instance of the unrolled loop (the rolled loop tests the pointer per step): the same
    inline-asm FMA chains, explicit fmaf and DPP adds in the same order, only the stores differ -- y, h_out, c_out are bit-identical
    to the stash launch; so are they when h_out / c_out ARE h_in / c_in (the state is read before the first step)."""
    p = L.problem("default", 3, T)
    a, b, c = _fwd(dev, p), _fwd(dev, p, with_stash=False), _fwd(dev, p, with_stash=False, alias=True)
    for other in (b, c):
        assert _same(a["y"], other["y"]) and _same(a["h_out"], other["h_out"]) and _same(a["c_out"], other["c_out"])


def test_fwd_chunk_handover(dev):
    """272 steps in one launch == 256 then 16 through h_out / c_out, bit for bit (both ways run unrolled groups only; the state
    crosses the seam as the same fp32 numbers, in LDS / a register or through memory).  257 = 256 + 1 (the rolled loop behind
    the seam) satisfies the one-step gate across the seam."""
    for kind in ("default", "hot"):
        p = L.problem(kind, 3, 272)
        one = _fwd(dev, p)
        a = _fwd(dev, p, 0, 256)
        b = _fwd(dev, p, 256, 272, a["h_out"], a["c_out"])
        assert _same(one["stash"], np.concatenate([a["stash"], b["stash"]], 1))
        assert _same(one["y"], np.concatenate([a["y"], b["y"]], 1))
        assert _same(one["h_out"], b["h_out"]) and _same(one["c_out"], b["c_out"])
        p = L.problem(kind, 3, 257)
        a = _fwd(dev, p, 0, 256)
        b = _fwd(dev, p, 256, 257, a["h_out"], a["c_out"])
        out = L.fwd_gates(p, np.concatenate([a["stash"], b["stash"]], 1), np.concatenate([a["y"], b["y"]], 1), b["h_out"], b["c_out"])
        tol = 1.0
        assert max(out.values()) <= tol, (kind, out)


# ==== backward ====================================================================================================================
def _bwd(dev, p, entry, mode, dy=None):
    """entry l1 (mx_lstm_bwd_l1) | bwd (mx_lstm_bwd) | dgate (mx_lstm_bwd_dgate); mode l1 (wet + loss_scale) | dy.  The stash and y
    are the problem's (the fp64 forward rounded to fp32).  Returns (part (B, 17473), dgate (B, T, 256) or None)."""
    B, T = p["B"], p["T"]
    w = _weights(dev, p)
    x, lfo, y = RowsIn(dev, p["x"]), RowsIn(dev, p["lfo"]), RowsIn(dev, p["y"])
    tgt = RowsIn(dev, p["wet"] if mode == "l1" else (p["dy"] if dy is None else dy))
    stash, h0, c0 = dvc(dev, p["stash"]), dvc(dev, p["h_in"]), dvc(dev, p["c_in"])
    part = Out(dev, B * NPARAM)
    dgate = Out(dev, B * T * NG) if entry == "dgate" else None
    head = (x.ptr(), x.stride, lfo.ptr(), lfo.stride, y.ptr(), y.stride)
    tail = (stash, w["w_hh"], w["fc_w"], h0, c0)
    if entry == "l1":
        assert mode == "l1"
        call("mx_lstm_bwd_l1", *head, tgt.ptr(), tgt.stride, *tail, p["loss_scale"], part, B, T)
    elif entry == "bwd":
        assert mode == "dy"
        call("mx_lstm_bwd", *head, tgt.ptr(), tgt.stride, *tail, part, B, T)
    else:
        wet_args = (tgt.ptr(), tgt.stride, None, 0) if mode == "l1" else (None, 0, tgt.ptr(), tgt.stride)
        call("mx_lstm_bwd_dgate", *head, *wet_args, *tail, p["loss_scale"], part, dgate, B, T)
    assert part.guards_intact() and part.untouched() == 0                            # no sentinel left in part
    dg = None
    if dgate is not None:
        assert dgate.guards_intact() and dgate.untouched() == 0
        dg = dgate.read().reshape(B, T, NG)
    return part.read().reshape(B, NPARAM), dg


def _l1_grad32(p):
    """The L1 gradient as the caller of mx_lstm_bwd would hand it over: loss_scale sign(y - wet) in fp32, sign(0) = 0."""
    return (f32(p["loss_scale"]) * np.sign(p["y"] - p["wet"])).astype(f32)


BWD_T = [1, 2, 3, 4, 5, 31, 32, 33, 34, 63, 64, 65, 97, 129]


@pytest.mark.parametrize("T", BWD_T)
def test_bwd_contractive_running_bound(dev, T):
    """1 .. 5: the left-over pair alone, with and without dg(1) (x) h_0; 31 | 32 | 33 | 34: below, at and above one slab (33: the
    one-step last slab; 34: a two-step one); 63 | 64 | 65: the same one slab later (the double buffer has turned); 97 | 129: three
    and four full slabs behind a one-step one.  Five launches per clip count: the fused L1 kernel, mx_lstm_bwd with the same L1
    gradient as dy and with a random dy, mx_lstm_bwd_dgate with wet and with dy.  Every element of every per-clip row of part
    and of dgate within its running bound; the two bias rows bit-equal; the dy launch with the L1 gradient and the fused launch
    within the two bounds together.  The first and the last sample of every clip (and a quarter of the others) have y == wet
    exactly: their bound is zero, so dgate[T - 1] must be exactly zero, and at T = 1 all of part."""
    tol = 1.0
    for B in (1, 3):
        p = L.problem("contractive", B, T)
        ref = {m: L.running_ref("contractive", B, T, m) for m in ("l1", "dy")}
        assert p["ties"][:, 0].all() and p["ties"][:, -1].all() and not ref["l1"]["e_dgate"][:, -1].any()
        runs = {"l1": _bwd(dev, p, "l1", "l1"), "bwd_l1grad": _bwd(dev, p, "bwd", "dy", _l1_grad32(p)), "bwd_dy": _bwd(dev, p, "bwd", "dy"),
                "dgate_wet": _bwd(dev, p, "dgate", "l1"), "dgate_dy": _bwd(dev, p, "dgate", "dy")}
        for name, (part, dg) in runs.items():
            r = ref["dy" if name.endswith("dy") else "l1"]
            out = L.part_ratios(part, r["part"], r["e_part"])
            if dg is not None:
                out["dgate"] = L.ratio(dg, r["dgate"], r["e_dgate"])
            print("lstm64 bwd contractive", T, B, name, {k: round(v, 3) for k, v in out.items()})
            assert out["w_ih"] <= tol, (B, name, out)
            assert out["w_hh"] <= tol, (B, name, out)
            assert out["b_ih"] <= tol, (B, name, out)
            assert out["b_hh"] <= tol, (B, name, out)
            assert out["fc_w"] <= tol, (B, name, out)
            assert out["fc_b"] <= tol, (B, name, out)
            assert out.get("dgate", 0.0) <= tol, (B, name, out)
            assert out["bias"] == 0, (B, name)
        assert ratio(runs["l1"][0], runs["bwd_l1grad"][0], 2.0 * ref["l1"]["e_part"]) <= tol, B
        if T == 1:
            assert not runs["l1"][0].any() and not runs["dgate_wet"][0].any() and not runs["dgate_wet"][1].any()


@pytest.mark.parametrize("kind", ["default", "hot"])
@pytest.mark.parametrize("T", [1, 2, 33, 65, 257])
def test_bwd_dgate_local_step(dev, kind, T):
    """Weights on the product scale, where no running bound stays useful: dgate[t] against step_bwd from the DEVICE's dgate[t + 1]
    (dc is carried by the reference), part against the fp64 sums of the device's dgate.  257: eight full slabs behind a one-step one."""
    tol = 1.0
    for B in (1, 3):
        p = L.problem(kind, B, T)
        for mode in ("l1", "dy"):
            part, dg = _bwd(dev, p, "dgate", mode)
            g = L.loss_grad(p, p["y"], mode)
            r = L.step_bwd(p, p["stash"], p["y"], g, dg)
            out = L.part_ratios(part, *L.part_from_dgate(p, p["stash"], p["y"], g, dg))
            out["dgate"] = L.ratio(dg, r["dgate"], r["e_dgate"])
            print("lstm64 bwd local", kind, T, B, mode, {k: round(v, 3) for k, v in out.items()})
            assert out["dgate"] <= tol, (B, mode, out)
            assert out["w_ih"] <= tol, (B, mode, out)
            assert out["w_hh"] <= tol, (B, mode, out)
            assert out["b_ih"] <= tol, (B, mode, out)
            assert out["fc_w"] <= tol, (B, mode, out)
            assert out["fc_b"] <= tol, (B, mode, out)
            assert out["bias"] == 0, (B, mode)


R_TRAIN = 4.0


@pytest.mark.parametrize("T", [24, 257])
def test_bwd_training_kernel_yardstick(dev, T):
    """The helper-wave kernel behind mx_lstm_bwd_l1 / mx_lstm_bwd leaves no dgate, so on the default set (product-scale weights)
    no bound derives for it.  Yardstick of test_lstmg_recurrence, per parameter tensor and PER CLIP ROW:
    err <= R max(e32, u max|ref|), e32 = the error of the helper's fp32 emulation (emu_bwd) against the same fp64 reference.

    Measured on the MI355X, worst err / max(e32, floor) over the clips and both entry points:
        T = 24    l1:  w_ih 0.97  w_hh 0.95  b_ih = b_hh 1.38  fc_w 1.39  fc_b 1.00
                  dy:  w_ih 1.02  w_hh 1.25  b_ih = b_hh 1.00  fc_w 0.71  fc_b 1.00
        T = 257   l1:  w_ih 0.80  w_hh 1.33  b_ih = b_hh 1.06  fc_w 1.50  fc_b 1.00
                  dy:  w_ih 0.49  w_hh 1.01  b_ih = b_hh 1.52  fc_w 1.13  fc_b 1.00
    (1.00: the kernel's sum came out as the emulation's.)  Twice the worst (1.52) rounded up to a power of two: R = 4, below the
    8 the generic LSTM needed: the kernel's exact-fp32 matrix products and fused multiply-adds cost no more than numpy's fp32
    run of the same formulae.
    """
    B = 3
    p = L.problem("default", B, T)
    worst = {}
    for entry, mode in (("l1", "l1"), ("bwd", "dy")):
        part, _ = _bwd(dev, p, entry, mode)
        g = L.loss_grad(p, p["y"], mode)
        r = L._bptt(p, p["stash"], p["y"], g)
        ref = L._part(p, p["stash"], r["dgate"], r["e_dgate"], r["s_dgate"], r["dzy"], r["e_dzy"])[0]
        emu = L.emu_bwd(p, p["stash"], p["y"], mode)[1]
        assert np.isfinite(part).all()
        for name, (lo, hi) in L.PARTS.items():
            for b in range(B):
                err = float(np.abs(part[b, lo:hi].astype(f64) - ref[b, lo:hi]).max())
                e32 = float(np.abs(emu[b, lo:hi].astype(f64) - ref[b, lo:hi]).max())
                worst[(entry, name)] = max(worst.get((entry, name), 0.0), err / max(e32, U * float(np.abs(ref[b, lo:hi]).max()), 1e-300))
        assert np.array_equal(bits(part[:, slice(*L.PARTS["b_ih"])]), bits(part[:, slice(*L.PARTS["b_hh"])]))
    print("lstm64 bwd yardstick", T, {f"{k[0]}.{k[1]}": round(v, 3) for k, v in worst.items()})
    tol = R_TRAIN
    for key, v in worst.items():
        assert v <= tol, (key, worst)


# ==== mx_lstm_dlfo, mx_reduce_rows ================================================================================================
@pytest.mark.parametrize("B,T", [(1, 1), (3, 33), (3, 257), (1, 6)])
def test_dlfo(dev, B, T):
    """dlfo[b][t] = sum_r w_ih[r][0] dgate[b][t][r] against the fp64 dot products, gamma(256 + 2) of the magnitudes.  B T = 1, 99,
    771, 6: never a multiple of the four (b, t) a workgroup takes; dlfo_stride > T, the gaps untouched."""
    assert (B * T) % 4
    p = L.problem("hot", B, T)
    g = np.random.default_rng(B * 1000 + T)
    dgate = (g.standard_normal((B, T, NG)) * np.exp(g.uniform(-6, 0, (B, T, 1)))).astype(f32)
    out = RowsOut(dev, B, T)
    call("mx_lstm_dlfo", dv(dev, dgate), dvc(dev, p["w_ih"]), B, T, out.ptr(), out.stride)
    got, clean = out.read()
    assert clean
    ref, bound = L.dlfo64(p, dgate)
    tol = 1.0
    assert ratio(got, ref, bound) <= tol


@pytest.mark.parametrize("R", [1, 3])
def test_reduce_rows_on_part(dev, R):
    """No kernel-level test pins mx_reduce_rows (tests/test_gpu_lstm.py uses it as the reference of the fused optimizer step), so it
    is held here on gradient rows: the column sums are formed in fp64 and rounded once (u / 2 of |sum|, charged u); accumulate = 1
    adds that to out in fp32: u |out| more.  C = 17473 is no multiple of the 16 columns of a workgroup."""
    g = np.random.default_rng(R)
    part = (g.standard_normal((R, NPARAM)) * np.exp(g.uniform(-8, 2, (R, NPARAM)))).astype(f32)
    prev = g.standard_normal(NPARAM).astype(f32)
    s = part.astype(f64).sum(0)
    tol = 1.0
    for accumulate in (0, 1):
        out = Out(dev, NPARAM, init=prev if accumulate else None)
        call("mx_reduce_rows", dv(dev, part), R, NPARAM, accumulate, out)
        assert out.guards_intact() and out.untouched() == 0
        ref = s + prev.astype(f64) if accumulate else s
        bound = U * np.abs(s) + (U * np.abs(ref) if accumulate else 0.0)
        assert ratio(out.read(), ref, bound) <= tol, accumulate


# ==== documented statuses, before any launch ==========================================================================================
def test_argument_statuses(dev):
    """Every required pointer NULL, B = 0, T = 0 -> ARG; mx_lstm_bwd / mx_lstm_bwd_dgate with dy_stride < T, mx_lstm_bwd_dgate with
    both or neither of wet / dy or without dgate, mx_lstm_dlfo with dlfo_stride < T -> ARG; T = 2^30 -> UNSUPPORTED.  Nothing is
    launched: every output keeps its sentinels."""
    B, T = 1, 2
    p = L.problem("default", B, T)
    w = _weights(dev, p)
    rows = {n: RowsIn(dev, p[n]) for n in ("x", "lfo", "y", "wet", "dy")}
    st = rows["x"].stride
    stash_in, h0, c0 = dvc(dev, p["stash"]), dvc(dev, p["h_in"]), dvc(dev, p["c_in"])
    outs = dict(h=Out(dev, B * H), c=Out(dev, B * H), y=Out(dev, 16), stash=Out(dev, B * T * STASH), part=Out(dev, B * NPARAM),
                dgate=Out(dev, B * T * NG), dlfo=Out(dev, 16))
    r = {n: v.ptr() for n, v in rows.items()}
    ok = {
        "mx_lstm_fwd": [r["x"], st, r["lfo"], st, w["w_ih"], w["w_hh"], w["b_ih"], w["b_hh"], w["fc_w"], w["fc_b"], h0, c0, outs["h"],
                        outs["c"], outs["y"], st, outs["stash"], B, T],
        "mx_lstm_bwd_l1": [r["x"], st, r["lfo"], st, r["y"], st, r["wet"], st, stash_in, w["w_hh"], w["fc_w"], h0, c0, 0.5, outs["part"], B, T],
        "mx_lstm_bwd": [r["x"], st, r["lfo"], st, r["y"], st, r["dy"], st, stash_in, w["w_hh"], w["fc_w"], h0, c0, outs["part"], B, T],
        "mx_lstm_bwd_dgate": [r["x"], st, r["lfo"], st, r["y"], st, r["wet"], st, None, 0, stash_in, w["w_hh"], w["fc_w"], h0, c0, 0.5,
                              outs["part"], outs["dgate"], B, T],
        "mx_lstm_dlfo": [stash_in, w["w_ih"], B, T, outs["dlfo"], st],
    }
    ptrs = {"mx_lstm_fwd": [0, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14], "mx_lstm_bwd_l1": [0, 2, 4, 6, 8, 9, 10, 11, 12, 14],
            "mx_lstm_bwd": [0, 2, 4, 6, 8, 9, 10, 11, 12, 13], "mx_lstm_bwd_dgate": [0, 2, 4, 10, 11, 12, 13, 14, 16, 17],
            "mx_lstm_dlfo": [0, 1, 4]}
    bt = {"mx_lstm_fwd": (17, 18), "mx_lstm_bwd_l1": (15, 16), "mx_lstm_bwd": (14, 15), "mx_lstm_bwd_dgate": (18, 19), "mx_lstm_dlfo": (2, 3)}

    def with_(name, **kw):
        a = list(ok[name])
        for i, v in kw.items():
            a[int(i[1:])] = v
        return a
    for name, args in ok.items():
        for i in ptrs[name]:
            assert status(name, *with_(name, **{f"i{i}": None})) == ARG, (name, i)
        for i in bt[name]:
            assert status(name, *with_(name, **{f"i{i}": 0})) == ARG, (name, i)
    assert status("mx_lstm_bwd", *with_("mx_lstm_bwd", i7=T - 1)) == ARG
    dg = "mx_lstm_bwd_dgate"
    assert status(dg, *with_(dg, i8=r["dy"], i9=st)) == ARG                                         # both wet and dy
    assert status(dg, *with_(dg, i6=None)) == ARG                                                   # neither
    assert status(dg, *with_(dg, i6=None, i8=r["dy"], i9=T - 1)) == ARG                             # dy_stride < T
    assert status("mx_lstm_dlfo", *with_("mx_lstm_dlfo", i5=T - 1)) == ARG
    big = 1 << 30
    assert status("mx_lstm_fwd", *with_("mx_lstm_fwd", i18=big)) == UNSUPPORTED
    assert status("mx_lstm_bwd_l1", *with_("mx_lstm_bwd_l1", i16=big)) == UNSUPPORTED
    assert status("mx_lstm_bwd", *with_("mx_lstm_bwd", i7=big, i15=big)) == UNSUPPORTED
    assert status(dg, *with_(dg, i19=big)) == UNSUPPORTED
    torch.cuda.synchronize()
    for name, o in outs.items():
        assert o.guards_intact() and o.untouched() == o.words, name

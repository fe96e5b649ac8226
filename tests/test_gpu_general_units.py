"""GPU: the "general" kernels called on their raw entry points and held to the independent fp64 references of
tests/helpers/general_refs64.py -- mx_sgemm_f32, the im2col / col2im gathers, the row / channel / plane normalisations,
pool + PReLU, the bin-mean head, FiLM and the mx_lstmg_* recurrence (tcn.hip, cnn_generic.hip, tcn_general.hip,
lstm_generic.hip).  Until now they were reached only through whole models, against fp32 torch at 1e-5 of a tensor's maximum.

Stray writes: every output lives between two guard bands of 64 floats; outputs and guards are pre-filled with a NaN bit
pattern, and after the call every element the ABI does not promise to write must still hold its bits (guards, gaps of a
strided C, rows / columns beyond M / N, pad columns of a plane).  Observed, never provoked: every launch has valid arguments.

Tolerances (u = 2^-23, one fp32 ulp of 1; an fp32 operation rounds by at most u / 2 of its result):
* exact: integer-valued GEMMs (every partial sum < 2^24), the gathers, single-rounding outputs (a + b, a * b: the fp64 result
  rounded once to fp32 is the correctly rounded fp32 result) -- bit equality;
* sums: n u / (1 - n u) (sum of the magnitudes of the terms), n = the number of terms + 1 -- any summation order;
* reductions the kernels keep in fp64 and round once: u |ref| + 2^-40 sum |terms|;
* elementwise formulae: k u (sum of the magnitudes of the terms), k = the fp32 operations of the formula, beside each assert;
* the LSTM recurrence compounds its error over the steps: err <= R max(e32, u max|ref|), e32 = the error of the helper's own
  fp32 run of the same formulae on the same inputs.  R = 8: see test_lstmg_recurrence.
Every gate is asserted as ``worst ratio to its bound <= tol`` so the measured margin lands in measured_errors.json.
"""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import general_refs64 as G

pytestmark = pytest.mark.gpu

GUARD = 64                                   # floats on each side of every output
SENT = 0x7FC5A5A5                            # a quiet NaN with a payload: no kernel here produces it
U = 2.0 ** -23
POISON = np.float32(1.0e30)                  # fills the gaps of strided operands: must never reach a result
f32, f64 = np.float32, np.float64


def _hip():
    from mod_extraction_amd import _hip as h
    return h


class Buf:
    """A device output of n elements between guard bands, pre-filled with the sentinel (or ``init`` bits where given)."""

    def __init__(self, dev, n, init=None, dtype=f32):
        self.n, self.dtype = int(n), dtype
        if dtype == f32:
            full = np.full(self.n + 2 * GUARD, SENT, np.int32)
            self.g = GUARD
        else:                                                            # uint8 (argmax planes): 256 guard bytes
            full = np.full(self.n + 8 * GUARD, 0xA5, np.uint8)
            self.g = 4 * GUARD
        if init is not None:
            full[self.g:self.g + self.n] = np.ascontiguousarray(init, dtype).ravel().view(full.dtype)
        self.before = full.copy()
        self.t = torch.from_numpy(full).to(dev)

    def ptr(self, off=0):
        return self.t.data_ptr() + (self.g + off) * self.t.element_size()

    def read(self):
        torch.cuda.synchronize()
        self.after = self.t.cpu().numpy()
        return self.after[self.g:self.g + self.n].view(self.dtype).copy()

    def stray(self, written=None):
        """Number of elements outside ``written`` (flat bool over the body; None = the whole body) whose bits changed."""
        keep = np.ones(self.after.size, bool)
        body = np.ones(self.n, bool) if written is None else np.asarray(written, bool).ravel()
        keep[self.g:self.g + self.n] = ~body
        return int((self.after[keep] != self.before[keep]).sum())


def sent_f32(shape):
    return np.full(shape, SENT, np.int32).view(f32)


def dv(dev, a, dtype=f32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)


def ratio(got, ref, bound):
    """Worst |got - ref| / bound (0 where the difference is 0, so a zero bound demands equality; NaN if got has one)."""
    err = np.abs(np.asarray(got, f64) - np.asarray(ref, f64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / np.maximum(np.asarray(bound, f64), 1e-300))
    return float(np.max(r)) if r.size else 0.0


def fp64_once(ref, mag):
    """Bound of a reduction accumulated in fp64 and rounded once to fp32."""
    return U * np.abs(ref) + 2.0 ** -40 * np.asarray(mag, f64)


def call(name, *args):
    h = _hip()
    h.call(name, *[h.ptr(a) if isinstance(a, torch.Tensor) else a for a in args], h.stream())


def status(name, *args):
    h = _hip()
    return getattr(h.load(), name)(*[h.ptr(a) if isinstance(a, torch.Tensor) else a for a in args], h.stream())


def rnd(g, shape, scale=1.0):
    return (g.standard_normal(shape) * scale).astype(f32)


# ==== mx_sgemm_f32 ===========================================================================================================
def _layout(rows, cols, trans, inner, pad):
    """Element strides of a rows x cols operand: ``inner`` between neighbours of the fast axis, the slow axis padded."""
    if trans:
        rs, cs = inner, rows * inner + pad
    else:
        rs, cs = cols * inner + pad, inner
    return rs, cs, (rows - 1) * rs + (cols - 1) * cs + 1


def _gemm_spec(M, N, K, at=False, bt=False, ct=False, a_s=1, b_s=1, c_s=1, a_off=0, b_off=0, a_b0=False, b_b0=False, nb=1,
               pg=1, acc=0):
    a_rs, a_cs, a_span = _layout(M, K, at, a_s, 0 if a_s == 1 else 3)
    b_rs, b_cs, b_span = _layout(K, N, bt, b_s, 0 if b_s == 1 else 2)
    c_rs, c_cs, c_span = _layout(M, N, ct, c_s, 0 if c_s == 1 else 1)
    a_bs, b_bs, c_bs = (0 if a_b0 else a_span + 5), (0 if b_b0 else b_span + 3), c_span + 7
    groups = -(-nb // pg)
    return dict(M=M, N=N, K=K, nb=nb, pg=pg, acc=acc, a_off=a_off, a_rs=a_rs, a_cs=a_cs, a_bs=a_bs,
                a_len=a_off + (nb - 1) * a_bs + a_span, b_off=b_off, b_rs=b_rs, b_cs=b_cs, b_bs=b_bs,
                b_len=b_off + (nb - 1) * b_bs + b_span, c_off=0, c_rs=c_rs, c_cs=c_cs, c_bs=c_bs, c_len=(groups - 1) * c_bs + c_span)


def _tcn_res_dgrad(B=2, cin=5, cout=6, stride=2, t_out=173):
    """tcn.py: dxr (B, cin, 352)[.., t' stride] = res_w^T (cin, cout) dcur (B, cout, 352): C written with c_cs = stride."""
    P = G.PITCH
    return dict(M=cin, N=t_out, K=cout, nb=B, pg=1, acc=0, a_off=0, a_rs=1, a_cs=cin, a_bs=0, a_len=cout * cin, b_off=0, b_rs=P,
                b_cs=1, b_bs=cout * P, b_len=B * cout * P, c_off=0, c_rs=P, c_cs=stride, c_bs=cin * P, c_len=B * cin * P)


def _cnn_head_wgrad(B=3, L=3, C=7, W=37):
    """cnn_generic.py: dwo (L, C) = sum over clips of ds (B, L, W) latent (B, C, W)^T: per_group = B, one C slice."""
    return dict(M=L, N=C, K=W, nb=B, pg=B, acc=0, a_off=0, a_rs=W, a_cs=1, a_bs=L * W, a_len=B * L * W, b_off=0, b_rs=1, b_cs=W,
                b_bs=C * W, b_len=B * C * W, c_off=0, c_rs=C, c_cs=1, c_bs=0, c_len=L * C)


def _lstm_whh_wgrad(B=2, Hn=7, Tn=6):
    """lstm_generic.py: part (B, G, Hn) = dgate[:, 1:]^T (the dgate + G pointer) h[:, :-1] (the stash's h column): K = Tn - 1."""
    Gn = 4 * Hn
    return dict(M=Gn, N=Hn, K=Tn - 1, nb=B, pg=1, acc=0, a_off=Gn, a_rs=1, a_cs=Gn, a_bs=Tn * Gn, a_len=B * Tn * Gn, b_off=5 * Hn,
                b_rs=6 * Hn, b_cs=1, b_bs=Tn * 6 * Hn, b_len=B * Tn * 6 * Hn, c_off=0, c_rs=Hn, c_cs=1, c_bs=Gn * Hn, c_len=B * Gn * Hn)


def _run_gemm(dev, s, exact, seed):
    g = np.random.default_rng(seed)

    def values(n):
        if exact:
            return g.integers(-8, 9, n).astype(f32)
        return (g.choice([-1.0, 1.0], n) * 2.0 ** g.uniform(-10, 3, n)).astype(f32)

    a, b, c0 = values(s["a_len"]), values(s["b_len"]), values(s["c_len"])
    if exact:
        c0[c0 == 0] = 5.0
    m, n, k = np.arange(s["M"]), np.arange(s["N"]), np.arange(s["K"])
    for buf, off, rs, cs, bs, r, c in ((a, s["a_off"], s["a_rs"], s["a_cs"], s["a_bs"], m, k),
                                       (b, s["b_off"], s["b_rs"], s["b_cs"], s["b_bs"], k, n)):
        used = np.zeros(buf.size, bool)
        for i in range(s["nb"]):
            used[off + i * bs + r[:, None] * rs + c[None, :] * cs] = True
        buf[~used] = POISON                                             # whatever the GEMM must not read
    args = (s["a_rs"], s["a_cs"], s["a_bs"]), (s["b_rs"], s["b_cs"], s["b_bs"]), (s["c_rs"], s["c_cs"], s["c_bs"])
    ref, written, mag, summed = G.sgemm(a, s["a_off"], *args[0], b, s["b_off"], *args[1], c0, s["c_off"], *args[2], s["M"], s["N"],
                                        s["K"], s["nb"], s["pg"], s["acc"])
    init = sent_f32(s["c_len"])
    if s["acc"]:
        init[written] = c0[written]
    out = Buf(dev, s["c_len"], init)
    at, bt = dv(dev, a), dv(dev, b)
    h = _hip()
    h.call("mx_sgemm_f32", at.data_ptr() + 4 * s["a_off"], *args[0], bt.data_ptr() + 4 * s["b_off"], *args[1], out.ptr(s["c_off"]),
           *args[2], s["M"], s["N"], s["K"], s["nb"], s["pg"], s["acc"], h.stream())
    got = out.read()
    return got, ref, written, mag, summed, out


_E = [
    ("rm_1x1x1", (1, 1, 1), {}), ("rm_31x33x17", (31, 33, 17), {}), ("rm_32x32x16", (32, 32, 16), {}),
    ("rm_33x31x15", (33, 31, 15), {}), ("rm_63x65x3", (63, 65, 3), {}), ("rm_64x64x2", (64, 64, 2), {}),
    ("rm_65x63x33", (65, 63, 33), {}), ("rm_130x130x100", (130, 130, 100), {}), ("rm_1x130x33", (1, 130, 33), {}),
    ("rm_130x1x100", (130, 1, 100), {}),
    ("at_33x65x17", (33, 65, 17), dict(at=True)), ("at_64x31x1", (64, 31, 1), dict(at=True)),
    ("at_130x32x15", (130, 32, 15), dict(at=True)),
    ("bt_65x33x3", (65, 33, 3), dict(bt=True)), ("bt_31x64x100", (31, 64, 100), dict(bt=True)), ("bt_1x63x16", (1, 63, 16), dict(bt=True)),
    ("atbt_63x130x33", (63, 130, 33), dict(at=True, bt=True)),
    ("s23_33x31x17", (33, 31, 17), dict(a_s=2, b_s=3)), ("s32t_65x64x15", (65, 64, 15), dict(at=True, bt=True, a_s=3, b_s=2)),
    ("s23_32x1x2", (32, 1, 2), dict(a_s=2, b_s=3)),
    ("abcast_63x33x16_nb3", (63, 33, 16), dict(a_b0=True, nb=3)), ("bbcast_31x65x33_nb3", (31, 65, 33), dict(b_b0=True, nb=3)),
    ("off13_64x63x17", (64, 63, 17), dict(a_off=1, b_off=3)), ("off31_at_33x32x100", (33, 32, 100), dict(at=True, a_off=3, b_off=1)),
    ("off13_bt_130x31x1", (130, 31, 1), dict(bt=True, a_off=1, b_off=3)),
    ("ccs3_65x33x15", (65, 33, 15), dict(c_s=3)), ("ccs3_1x64x17", (1, 64, 17), dict(c_s=3)),
    ("crs1_63x65x16", (63, 65, 16), dict(ct=True)), ("crs3_31x130x3", (31, 130, 3), dict(ct=True, c_s=3)),
    ("nb3_pg1_33x33x17", (33, 33, 17), dict(nb=3, pg=1)), ("nb3_pg2_64x31x15", (64, 31, 15), dict(nb=3, pg=2)),
    ("nb3_pg3_31x64x33", (31, 64, 33), dict(nb=3, pg=3)), ("nb5_pg1_32x65x2", (32, 65, 2), dict(nb=5, pg=1)),
    ("nb5_pg2_65x32x100", (65, 32, 100), dict(nb=5, pg=2)), ("nb5_pg5_63x63x16", (63, 63, 16), dict(nb=5, pg=5)),
    ("nb1_pg2_33x1x3", (33, 1, 3), dict(nb=1, pg=2)),
    ("acc_65x65x17", (65, 65, 17), dict(acc=1)), ("acc_nb5_pg2_31x33x33", (31, 33, 33), dict(acc=1, nb=5, pg=2)),
    ("acc_nb3_pg3_at_64x64x15", (64, 64, 15), dict(acc=1, nb=3, pg=3, at=True)), ("acc_ccs3_33x63x100", (33, 63, 100), dict(acc=1, c_s=3)),
    ("acc_nb5_pg1_1x31x16", (1, 31, 16), dict(acc=1, nb=5, pg=1)),
]
_SITES = [("site_tcn_res_dgrad_ccs_stride", _tcn_res_dgrad), ("site_cnn_head_wgrad_per_group_B", _cnn_head_wgrad),
          ("site_lstm_whh_wgrad_offset_K_Tn_1", _lstm_whh_wgrad)]
_EXACT = [pytest.param(lambda mnk=mnk, kw=kw: _gemm_spec(*mnk, **kw), id=name) for name, mnk, kw in _E] + \
         [pytest.param(fn, id=name) for name, fn in _SITES]


@pytest.mark.parametrize("spec", _EXACT)
def test_sgemm_exact_on_integers(dev, spec):
    """Operands are integers in [-8, 8]: every product and partial sum is exact in fp32 (K x batches summed <= 5000,
    |sum| <= 320 000 < 2^24), so the result must equal the fp64 reference bit for bit whatever the summation order --
    one wrong tail element, one dropped k term or one poison value read from a gap shows."""
    s = spec()
    assert s["K"] * min(s["pg"], s["nb"]) <= 5000
    got, ref, written, _, _, out = _run_gemm(dev, s, True, 1234)
    assert written.sum() == s["M"] * s["N"] * -(-s["nb"] // s["pg"])
    assert out.stray(written) == 0, "a write outside the M x N elements of C (gap, tail or guard band)"
    bad = np.flatnonzero(bits(got)[written] != bits(ref.astype(f32))[written])
    assert bad.size == 0, (bad[:5], got[written][bad[:5]], ref[written][bad[:5]])


@pytest.mark.parametrize("mnk,kw", [
    pytest.param((65, 33, 100), {}, id="65x33x100"), pytest.param((33, 65, 1000), {}, id="33x65x1000"),
    pytest.param((64, 31, 100), dict(nb=5, pg=2, acc=1, at=True), id="at_nb5_pg2_acc_64x31x100"),
    pytest.param((31, 64, 1000), dict(nb=3, pg=3, acc=1, bt=True, c_s=3), id="bt_nb3_pg3_acc_ccs3_31x64x1000"),
    pytest.param((130, 63, 1000), dict(nb=3, pg=1, a_off=1, b_off=3), id="nb3_off_130x63x1000")])
def test_sgemm_rounding_bound_on_random_floats(dev, mnk, kw):
    """|x| in [2^-10, 8], no denormals.  |C - C64| <= n u / (1 - n u) (|A||B| + |C_in|), n = K x batches summed + 1: the inner
    product bound of any summation order with the truncation unit roundoff; a dropped term is ~ 1 / K of the sum."""
    s = _gemm_spec(*mnk, **kw)
    got, ref, written, mag, summed, out = _run_gemm(dev, s, False, 99)
    assert out.stray(written) == 0
    tol = 1.0
    assert ratio(got[written], ref[written], G.gamma(s["K"] * summed[written] + 1) * mag[written]) <= tol


# ==== gathers ===============================================================================================================
def _im2col_geoms(kh, kw):
    for dh, dw in ((1, 1), (2, 3)):
        for H in (1, 5):
            for W in (1, 7, 300):
                for nb in (1, 3):
                    for Cin in (1, 3):
                        yield nb, Cin, H, W, dh, dw, G.same_pad(kh, dh), G.same_pad(kw, dw)
    yield 3, 3, 5, 7, 2, 3, 2 * (kh - 1), 0                              # explicit padding: the causal case of tcn.py
    yield 1, 3, 1, 300, 1, 3, 0, 3 * (kw - 1)                            # one bin row, causal along the frames


@pytest.mark.parametrize("kh,kw", [(1, 1), (3, 3), (2, 4), (5, 13), (4, 1)])
def test_im2col2d_col2im2d(dev, kh, kw):
    """mx_im2col2d is a permutation with zero fill: bit equality.  mx_col2im2d sums at most kh kw terms: the rounding bound
    with n = kh kw against the reference transpose, and <col2im(dcol), x> == <dcol, im2col(x)> in fp64 to 1e-6 of the sum of
    the magnitudes of the products (the adjoint identity).  Even kernels: the asymmetric "same" padding; H = 1 / W = 1:
    dilation x (k - 1) >= the image, every tap but one outside; most sizes are no multiple of the 256-thread block."""
    g = np.random.default_rng(kh * 16 + kw)
    for nb, Cin, H, W, dh, dw, pt, pl in _im2col_geoms(kh, kw):
        Kk, P = Cin * kh * kw, nb * H * W
        x, dcol = rnd(g, (nb, Cin, H, W)), rnd(g, (Kk, P))
        col, dx = Buf(dev, Kk * P), Buf(dev, nb * Cin * H * W)
        call("mx_im2col2d", dv(dev, x), nb, Cin, H, W, kh, kw, dh, dw, pt, pl, col.ptr())
        call("mx_col2im2d", dv(dev, dcol), nb, Cin, H, W, kh, kw, dh, dw, pt, pl, dx.ptr())
        got_col, got_dx = col.read().reshape(Kk, P), dx.read().reshape(nb, Cin, H, W)
        where = (kh, kw, nb, Cin, H, W, dh, dw, pt, pl)
        assert col.stray() == 0 and dx.stray() == 0, where
        ref_col = G.im2col2d(x, kh, kw, dh, dw, pt, pl)
        assert np.array_equal(bits(got_col), bits(ref_col)), where
        ref_dx = G.col2im2d(dcol.astype(f64), nb, Cin, H, W, kh, kw, dh, dw, pt, pl)
        mag = G.col2im2d(np.abs(dcol).astype(f64), nb, Cin, H, W, kh, kw, dh, dw, pt, pl)
        tol = 1.0
        assert ratio(got_dx, ref_dx, G.gamma(kh * kw) * mag) <= tol, where
        lhs, rhs = float((got_dx.astype(f64) * x).sum()), float((dcol.astype(f64) * ref_col).sum())
        assert abs(lhs - rhs) <= 1e-6 * float(np.abs(dcol.astype(f64) * ref_col).sum()) + 1e-300, where


@pytest.mark.parametrize("ksz", [1, 3, 4, 9])
def test_tcn_im2col_col2im(dev, ksz):
    """Without statistics the gather is exact; with them every element is (x - mean) rstd, two roundings: <= 2 ulp of the fp64
    value.  mx_tcn_col2im (its divisibility test on the stride) under the rounding bound with n = ksz; it writes the T valid
    columns only.  T = 353 is beyond the plane: MX_ERR_ARG."""
    g = np.random.default_rng(ksz)
    B, C = 2, 3
    for dil in (1, 4):
        for stride in (1, 2, 3):
            for T in (1, 5, 352):
                To = G.conv1d_out_len(T, ksz, dil, stride)
                x = sent_f32((B, C, G.PITCH))                             # pad columns: never to be read
                x[:, :, :T] = rnd(g, (B, C, T), 2.0) + 0.5
                stats = np.stack([x[:, :, :T].astype(f64).mean((1, 2)), 1 / np.sqrt(x[:, :, :T].astype(f64).var((1, 2)) + 1e-5)], -1).astype(f32)
                where = (ksz, dil, stride, T, To)
                for st in (None, stats):
                    col = Buf(dev, C * ksz * B * To)
                    call("mx_tcn_im2col", dv(dev, x), None if st is None else dv(dev, st), B, C, T, To, ksz, dil, stride, col.ptr())
                    got = col.read().reshape(C * ksz, B * To)
                    assert col.stray() == 0, where
                    ref = G.tcn_im2col(x, st, T, To, ksz, dil, stride)
                    if st is None:
                        assert np.array_equal(bits(got), bits(ref)), where
                    else:
                        tol = 1.0
                        assert ratio(got, ref, 2 * U * np.abs(ref)) <= tol, where            # k = 2: subtract, multiply
                dcol = rnd(g, (C * ksz, B * To))
                dx = Buf(dev, B * C * G.PITCH)
                call("mx_tcn_col2im", dv(dev, dcol), B, C, T, To, ksz, dil, stride, dx.ptr())
                got = dx.read().reshape(B, C, G.PITCH)
                valid = np.zeros((B, C, G.PITCH), bool)
                valid[:, :, :T] = True
                assert dx.stray(valid) == 0, where
                ref = G.tcn_col2im(dcol.astype(f64), B, C, T, To, ksz, dil, stride)
                mag = G.tcn_col2im(np.abs(dcol).astype(f64), B, C, T, To, ksz, dil, stride)
                tol = 1.0
                assert ratio(got[:, :, :T], ref, G.gamma(ksz) * mag) <= tol, where
    big = torch.zeros(1 << 16, device=dev)
    assert status("mx_tcn_im2col", big, None, 1, 1, 353, 353, ksz, 1, 1, big) == -1
    assert status("mx_tcn_col2im", big, 1, 1, 353, 353, ksz, 1, 1, big) == -1


# ==== row LayerNorm, row sums ==================================================================================================
def _planted_rows(g, rows, n):
    x = rnd(g, (rows, n), 3.0) + 1.0
    if rows >= 3:
        x[1] = rnd(g, n, 1e-3)
        x[1, n // 2] = 1.0e4                                              # one huge among tiny: a one-pass variance cancels here
        x[2] = f32(3.7)                                                   # constant: rstd = 1 / sqrt(eps)
    return x


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1000])
def test_rowln_and_row_sums(dev, rows, n):
    g = np.random.default_rng(rows * 1000 + n)
    eps = 1e-5
    x, dy = _planted_rows(g, rows, n), rnd(g, (rows, n))
    x64 = x.astype(f64)
    y, st, sm = Buf(dev, rows * n), Buf(dev, rows * 2), Buf(dev, rows)
    call("mx_rowln_fwd", dv(dev, x), rows, n, eps, y.ptr(), st.ptr())
    call("mx_row_sums", dv(dev, x), rows, n, sm.ptr())
    gy, gst, gsm = y.read().reshape(rows, n), st.read().reshape(rows, 2), sm.read()
    assert y.stray() == 0 and st.stray() == 0 and sm.stray() == 0
    ry, rst = G.rowln_fwd(x, f64(f32(eps)))
    tol = 1.0
    s, smag = G.row_sums(x)
    assert ratio(gsm, s, fp64_once(s, smag)) <= tol
    assert ratio(gst[:, 0], rst[:, 0], fp64_once(rst[:, 0], smag / n)) <= tol
    assert ratio(gst[:, 1], rst[:, 1], (U + 2.0 ** -40) * rst[:, 1]) <= tol          # var is a sum of positive terms
    if rows >= 3:
        assert ratio(gst[2, 1], 1 / np.sqrt(f64(f32(eps))), U / np.sqrt(eps)) <= tol and not gy[2].any()
    # y = (x - mu) rstd with the fp32 statistics: round mu, round rstd, subtract, multiply: k = 4
    assert ratio(gy, ry, 4 * U * (np.abs(x64) + np.abs(rst[:, :1])) * rst[:, 1:]) <= tol
    dx = Buf(dev, rows * n)
    call("mx_rowln_bwd", dv(dev, dy), dv(dev, gy), dv(dev, gst), rows, n, dx.ptr())
    gdx = dx.read().reshape(rows, n)
    assert dx.stray() == 0
    rdx, (m1, m2) = G.rowln_bwd(dy, gy, gst)
    rstd, d64, y64 = gst[:, 1:].astype(f64), dy.astype(f64), gy.astype(f64)
    # rstd (g - m1 - y m2): multiply, two subtractions, multiply = 4 operations (the roundings of m1, m2 fit the half-ulp slack)
    assert ratio(gdx, rdx, 4 * U * rstd * (np.abs(d64) + np.abs(m1) + np.abs(y64 * m2))) <= tol


# ==== TCN planes: bias + PReLU + residual, LayerNorm backward ==========================================================================
@pytest.mark.parametrize("T", [1, 345, 352])
@pytest.mark.parametrize("B,C,opts", [(1, 1, "bsr"), (3, 5, "bsr"), (3, 5, "bs"), (1, 5, "br"), (3, 1, "sr")])
def test_tcn_act_fwd_bwd(dev, T, B, C, opts):
    """opts: b = bias, s = slope, r = residual / add given (else NULL).  Columns [T, 352) of y and dz are exact zeros; the pad
    columns of z are not touched; zb = z + bias is one rounding: bit equality."""
    g = np.random.default_rng(T * 100 + B * 10 + C)
    P = G.PITCH
    valid = np.zeros((B, C, P), bool)
    valid[:, :, :T] = True
    z, res = sent_f32((B, C, P)), sent_f32((B, C, P))
    z[valid], res[valid] = rnd(g, valid.sum()), rnd(g, valid.sum())
    bias = rnd(g, C) if "b" in opts else None
    slope = g.uniform(0.05, 0.5, C).astype(f32) if "s" in opts else None
    r = res if "r" in opts else None
    zbuf, y = Buf(dev, z.size, z), Buf(dev, z.size)
    call("mx_tcn_act_fwd", zbuf.ptr(), None if bias is None else dv(dev, bias), None if slope is None else dv(dev, slope),
         None if r is None else dv(dev, r), B, C, T, y.ptr())
    gz, gy = zbuf.read().reshape(B, C, P), y.read().reshape(B, C, P)
    assert zbuf.stray(valid) == 0 and y.stray() == 0
    zb, ry = G.tcn_act_fwd(np.where(valid, z, 0), bias, slope, None if r is None else np.where(valid, r, 0), T)
    assert np.array_equal(bits(gz[:, :, :T]), bits(zb.astype(f32)))
    assert not bits(gy[:, :, T:]).any()
    a = 1.0 if slope is None else slope.astype(f64)[None, :, None]
    tol = 1.0
    # add the bias, multiply by the slope, add the residual: k = 3
    assert ratio(gy[:, :, :T], ry[:, :, :T], 3 * U * (np.abs(a * zb) + np.abs(zb) + (0 if r is None else np.abs(res[:, :, :T].astype(f64))))) <= tol
    # backward on a planted PReLU input: exact +0 and -0 take the slope branch (zb > 0 ? 1 : slope)
    zbp, dy = sent_f32((B, C, P)), sent_f32((B, C, P))
    zbp[valid], dy[valid] = rnd(g, valid.sum()), rnd(g, valid.sum())
    zbp[:, :, 0] = 0.0
    if T > 1:
        zbp[:, :, 1] = -0.0
    dz, part = Buf(dev, z.size), Buf(dev, B * C * 2)
    call("mx_tcn_act_bwd", dv(dev, dy), dv(dev, zbp), None if slope is None else dv(dev, slope), B, C, T, dz.ptr(), part.ptr())
    gdz, gpart = dz.read().reshape(B, C, P), part.read().reshape(B * C, 2)
    assert dz.stray() == 0 and part.stray() == 0
    rdz, rpart, mag = G.tcn_act_bwd(np.where(valid, dy, 0), np.where(valid, zbp, 0), slope, T)
    assert np.array_equal(bits(gdz), bits(rdz.astype(f32)))                 # dy or slope dy: one rounding; zeros beyond T
    rpart[:, 0] = rdz.astype(f32).astype(f64).sum(-1).ravel()               # the ABI's "row sums of dz": of the fp32 values it stores
    assert ratio(gpart, rpart, fp64_once(rpart, mag)) <= tol


@pytest.mark.parametrize("T", [1, 345, 352])
@pytest.mark.parametrize("B,C,with_add", [(1, 1, True), (3, 5, True), (3, 5, False)])
def test_tcn_ln_bwd(dev, T, B, C, with_add):
    g = np.random.default_rng(T + B + C)
    P = G.PITCH
    valid = np.zeros((B, C, P), bool)
    valid[:, :, :T] = True
    x, gx, add = sent_f32((B, C, P)), sent_f32((B, C, P)), sent_f32((B, C, P))
    x[valid], gx[valid], add[valid] = rnd(g, valid.sum(), 2.0) + 0.5, rnd(g, valid.sum()), rnd(g, valid.sum())
    xv = x[:, :, :T].astype(f64)
    stats = np.stack([xv.mean((1, 2)), 1 / np.sqrt(xv.var((1, 2)) + 1e-5)], -1).astype(f32)
    dx = Buf(dev, x.size)
    call("mx_tcn_ln_bwd", dv(dev, x), dv(dev, gx), dv(dev, stats), dv(dev, add) if with_add else None, B, C, T, dx.ptr())
    got = dx.read().reshape(B, C, P)
    assert dx.stray() == 0 and not bits(got[:, :, T:]).any()
    ref, (m1, m2), xh = G.tcn_ln_bwd(np.where(valid, x, 0), np.where(valid, gx, 0), stats, np.where(valid, add, 0) if with_add else None, T)
    mean, rstd = stats.astype(f64)[:, 0, None, None], stats.astype(f64)[:, 1, None, None]
    xh_mag = (np.abs(xv) + np.abs(mean)) * rstd
    mag = rstd * (np.abs(gx[:, :, :T].astype(f64)) + np.abs(m1) + xh_mag * np.abs(m2)) + (np.abs(add[:, :, :T].astype(f64)) if with_add else 0)
    tol = 1.0
    # xhat = (x - mean) rstd (2), xhat m2, two subtractions, times rstd, plus add: k = 7
    assert ratio(got[:, :, :T], ref[:, :, :T], 7 * U * mag) <= tol


# ==== MaxPool2d((p, 1)) + PReLU ================================================================================================
def _q(g, shape, step=2.0 ** -6, lim=4.0):
    """Values on a coarse grid: z + bias is exact in fp32 (and exact ties inside windows are common)."""
    return (np.round(g.uniform(-lim, lim, shape) / step) * step).astype(f32)


@pytest.mark.parametrize("p,H", [(1, 3), (2, 3), (3, 3), (2, 7), (3, 7), (1, 8), (2, 8), (3, 8)])
@pytest.mark.parametrize("B,C,W", [(1, 1, 1), (3, 5, 7), (1, 5, 300)])
def test_pool_prelu_fwd_bwd(dev, p, H, B, C, W):
    """Grid-valued z and bias: z + bias is exact, so v and amax must EQUAL the reference (first maximum of a window), out is one
    rounding.  Backward: dz routed to the winning row bit for bit, exact zeros elsewhere and on the H mod p dropped rows."""
    g = np.random.default_rng(p * 100 + H * 10 + W)
    planes, Hp = B * C, H // p
    z, bias, slope = _q(g, (planes, H, W)), _q(g, C), g.uniform(0.05, 0.5, C).astype(f32)
    z[:, :p, 0] = z[:, :1, 0]                                              # a whole window tied: row 0 must win
    if p == 3 and W > 1:
        z[:, 1, W - 1] = z[:, 2, W - 1] = z[:, 0, W - 1] + 1                  # rows 1 and 2 tied above row 0: row 1 must win
    v, out, am = Buf(dev, planes * Hp * W), Buf(dev, planes * Hp * W), Buf(dev, planes * Hp * W, dtype=np.uint8)
    call("mx_pool_prelu_fwd", dv(dev, z), dv(dev, bias), planes, C, H, W, p, dv(dev, slope), v.ptr(), out.ptr(), am.ptr())
    gv, gout, gam = v.read().reshape(planes, Hp, W), out.read().reshape(planes, Hp, W), am.read().reshape(planes, Hp, W)
    assert v.stray() == 0 and out.stray() == 0 and am.stray() == 0
    rv, rout, ram = G.pool_prelu_fwd(z, bias, C, p, slope)
    assert np.array_equal(gam, ram) and not gam[:, 0, 0].any()
    if p == 3 and W > 1:
        assert (gam[:, 0, W - 1] == 1).all()
    assert np.array_equal(bits(gv), bits(rv.astype(f32)))
    assert np.array_equal(bits(gout), bits(rout.astype(f32)))                # v or slope v: one rounding
    # backward with planted pooled values of exactly +0 and -0 (v <= 0: the slope branch and the slope gradient's mask)
    gr, vv = rnd(g, (planes, Hp, W)), rv.astype(f32)
    vv[:, 0, 0] = 0.0
    vv[:, Hp - 1, W - 1] = -0.0
    dz, part = Buf(dev, planes * H * W), Buf(dev, planes * 2)
    call("mx_pool_prelu_bwd", dv(dev, gr), dv(dev, vv), dv(dev, ram, np.uint8), planes, C, H, W, p, dv(dev, slope), dz.ptr(), part.ptr())
    gdz, gpart = dz.read().reshape(planes, H, W), part.read().reshape(planes, 2)
    assert dz.stray() == 0 and part.stray() == 0
    rdz, rpart, mag = G.pool_prelu_bwd(gr, vv, ram, C, H, p, slope)
    assert np.array_equal(bits(gdz), bits(rdz.astype(f32)))
    assert not bits(gdz[:, Hp * p:]).any()
    tol = 1.0
    rpart[:, 0] = rdz.astype(f32).astype(f64).sum((1, 2))                   # the ABI's "sum of dz": of the fp32 values it stores
    assert ratio(gpart, rpart, fp64_once(rpart, mag)) <= tol


def test_pool_prelu_bias_rounding_decides_the_winner_and_unsupported_sizes(dev):
    """z = {1, 1 + 2^-23} in one window.  With bias 1024 both sums round to 1025 (one rounding, ulp 2^-13): a tie, the first row
    wins; with bias 0 the second row is greater.  The comparison is made on the ROUNDED sums, so the reference runs in fp32."""
    C, H, W, p = 2, 2, 3, 2
    z = np.zeros((C, H, W), f32)
    z[:, 0], z[:, 1] = 1.0, np.nextafter(f32(1.0), f32(2.0))
    bias, slope = np.array([1024.0, 0.0], f32), np.array([0.25, 0.25], f32)
    v, out, am = Buf(dev, C * W), Buf(dev, C * W), Buf(dev, C * W, dtype=np.uint8)
    call("mx_pool_prelu_fwd", dv(dev, z), dv(dev, bias), C, C, H, W, p, dv(dev, slope), v.ptr(), out.ptr(), am.ptr())
    gv, gout, gam = v.read().reshape(C, 1, W), out.read().reshape(C, 1, W), am.read().reshape(C, 1, W)
    rv, rout, ram = G.pool_prelu_fwd(z, bias, C, p, slope, dtype=f32)
    assert (gam[0] == 0).all() and (gam[1] == 1).all() and np.array_equal(gam, ram)
    assert np.array_equal(bits(gv), bits(rv)) and (gv[0] == 1025.0).all() and np.array_equal(bits(gout), bits(rout))
    assert v.stray() == 0 and out.stray() == 0 and am.stray() == 0
    big = torch.zeros(1 << 16, device=dev)
    assert status("mx_pool_prelu_fwd", big, big, 2, 2, 3, 3, 4, big, big, big, big) == -2           # p > H
    assert status("mx_pool_prelu_fwd", big, big, 3, 2, 4, 3, 2, big, big, big, big) == -2           # planes % C != 0
    assert status("mx_pool_prelu_bwd", big, big, big, 2, 2, 3, 3, 4, big, big, big) == -2
    assert status("mx_pool_prelu_bwd", big, big, big, 3, 2, 4, 3, 2, big, big, big) == -2


# ==== bin-mean head ===========================================================================================================
@pytest.mark.parametrize("H", [1, 5])
@pytest.mark.parametrize("W", [1, 300])
@pytest.mark.parametrize("C,L", [(1, 1), (7, 3), (1, 3), (7, 1)])
def test_binmean_head_fwd_bwd(dev, H, W, C, L):
    g = np.random.default_rng(H * 1000 + W + C * 10 + L)
    B = 2
    x = rnd(g, (B, C, H, W))
    k = 1 / np.sqrt(C)
    wout, bout = g.uniform(-k, k, (L, C)).astype(f32), g.uniform(-k, k, L).astype(f32)        # nn.Conv1d's init scale
    lat, out = Buf(dev, B * C * W), Buf(dev, B * L * W)
    call("mx_binmean_head_fwd", dv(dev, x), B, C, H, W, dv(dev, wout), dv(dev, bout), L, lat.ptr(), out.ptr())
    glat, gout = lat.read().reshape(B, C, W), out.read().reshape(B, L, W)
    assert lat.stray() == 0 and out.stray() == 0
    rlat, _, _ = G.binmean_head_fwd(x, wout, bout)
    tol = 1.0
    # H - 1 additions and one division: an H-term summation bound
    assert ratio(glat, rlat, G.gamma(H) * np.abs(x.astype(f64)).sum(2) / H) <= tol
    # the sigmoid against fp64 on the latent the kernel wrote (gated above): 4 ulp of 1.  The C fused multiply-adds and the
    # bias round the pre-activation by <= (C + 1) u / 2 sum |terms|, of which a sigmoid (slope <= 1 / 4) passes a quarter.
    pre = np.einsum("lc,bcw->blw", wout.astype(f64), glat.astype(f64)) + bout.astype(f64)[None, :, None]
    assert ratio(gout, G.sigmoid(pre), 4 * U) <= tol
    d_out, d_lat = rnd(g, (B, L, W)), rnd(g, (B, C, W))
    for do, dl in ((d_out, d_lat), (d_out, None), (None, d_lat)):
        ds, dx = Buf(dev, B * L * W), Buf(dev, B * C * H * W)
        call("mx_binmean_head_bwd", None if do is None else dv(dev, do), None if dl is None else dv(dev, dl), dv(dev, gout), dv(dev, wout),
             B, C, H, W, L, ds.ptr(), dx.ptr())
        gds, gdx = ds.read().reshape(B, L, W), dx.read().reshape(B, C, H, W)
        assert ds.stray() == 0 and dx.stray() == 0
        rds, rdx, mag = G.binmean_head_bwd(do, dl, gout, wout, B, C, H, W)
        if do is None:
            assert not bits(gds).any()
        # d_out * o * (1 - o): subtract, two multiplications: k = 3 (1 - o is exact to half an ulp of 1 >= 1 - o)
        assert ratio(gds, rds, 3 * U * np.abs(rds)) <= tol
        # dx from the ds the kernel wrote: L fused multiply-adds and the division: k = L + 1
        dl64 = 0 if dl is None else dl.astype(f64)
        tot = dl64 + np.einsum("lc,blw->bcw", wout.astype(f64), gds.astype(f64))
        mag2 = np.abs(dl64) + np.einsum("lc,blw->bcw", np.abs(wout.astype(f64)), np.abs(gds.astype(f64)))
        assert ratio(gdx[:, :, 0], tot / H, (L + 1) * U * mag2 / H) <= tol
        assert ratio(gdx, rdx, (L + 4) * U * mag[:, :, None, :] / H) <= tol                          # ... and end to end (+ k = 3 of ds)
        assert (bits(gdx) == bits(gdx[:, :, :1])).all()                                              # identical on every bin


# ==== the per-channel pieces of the general TCN ===================================================================================
@pytest.mark.parametrize("T", [1, 2, 255, 256, 257, 1000])
@pytest.mark.parametrize("B,C", [(1, 1), (3, 5), (1, 5), (3, 1)])
def test_chan_norm_film_prelu_res(dev, T, B, C):
    g = np.random.default_rng(T * 10 + B + C)
    tol = 1.0
    z = rnd(g, (B, C, T), 2.0) + 0.7
    z64 = z.astype(f64)
    st = Buf(dev, C * 2)
    call("mx_chan_stats", dv(dev, z), B, C, T, st.ptr())
    gst = st.read().reshape(C, 2)
    assert st.stray() == 0
    rst, smag = G.chan_stats(z)
    assert ratio(gst, rst, fp64_once(rst, smag)) <= tol
    norm = np.stack([rst[:, 0], 1 / np.sqrt(rst[:, 1] + 1e-5)], -1).astype(f32)
    n64 = norm.astype(f64)
    xh = Buf(dev, z.size)
    call("mx_chan_norm_fwd", dv(dev, z), dv(dev, norm), B, C, T, xh.ptr())
    gxh = xh.read().reshape(B, C, T)
    assert xh.stray() == 0
    # (z - mean) rstd: k = 2
    assert ratio(gxh, G.chan_norm_fwd(z, norm), 2 * U * (np.abs(z64) + np.abs(n64[None, :, 0, None])) * n64[None, :, 1, None]) <= tol
    gr = rnd(g, (B, C, T))
    for train in (1, 0):
        dz = Buf(dev, z.size)
        call("mx_chan_norm_bwd", dv(dev, gr), dv(dev, gxh), dv(dev, norm), B, C, T, train, dz.ptr())
        gdz = dz.read().reshape(B, C, T)
        assert dz.stray() == 0
        rdz, (m1, m2) = G.chan_norm_bwd(gr, gxh, norm, train)
        mag = n64[None, :, 1, None] * (np.abs(gr.astype(f64)) + np.abs(m1) + np.abs(gxh.astype(f64) * m2))
        # train: rstd (g - m1 - xhat m2): k = 4;  eval: rstd g, one rounding (g - 0 - xhat 0 is exact)
        assert ratio(gdz, rdz, (4 if train else 1) * U * mag) <= tol
        if not train:
            assert np.array_equal(bits(gdz), bits(rdz.astype(f32)))
    gb = rnd(g, (B, 2 * C))
    a = Buf(dev, z.size)
    call("mx_film_fwd", dv(dev, gxh), dv(dev, gb), B, C, T, a.ptr())
    ga = a.read().reshape(B, C, T)
    assert a.stray() == 0
    gb64 = gb.astype(f64)
    # xhat gain + shift, not contracted: k = 2
    assert ratio(ga, G.film_fwd(gxh, gb), 2 * U * (np.abs(gxh.astype(f64) * gb64[:, :C, None]) + np.abs(gb64[:, C:, None]))) <= tol
    dxh, dgb = Buf(dev, z.size), Buf(dev, B * 2 * C)
    call("mx_film_bwd", dv(dev, gr), dv(dev, gxh), dv(dev, gb), B, C, T, dxh.ptr(), dgb.ptr())
    gdxh, gdgb = dxh.read().reshape(B, C, T), dgb.read().reshape(B, 2 * C)
    assert dxh.stray() == 0 and dgb.stray() == 0
    rdxh, rdgb, mag = G.film_bwd(gr, gxh, gb)
    assert np.array_equal(bits(gdxh), bits(rdxh.astype(f32)))               # da gain: one rounding
    assert ratio(gdgb, rdgb, fp64_once(rdgb, mag)) <= tol
    # PReLU + residual with planted +0 / -0 activations; slope = NULL and res = NULL where the ABI allows it
    act, res, slope = ga.copy(), rnd(g, (B, C, T)), g.uniform(0.05, 0.5, C).astype(f32)
    act[:, :, 0] = 0.0
    if T > 1:
        act[:, :, 1] = -0.0
    for sl, rs in ((slope, res), (None, res), (slope, None), (None, None)):
        y = Buf(dev, z.size)
        call("mx_prelu_res_fwd", dv(dev, act), None if sl is None else dv(dev, sl), None if rs is None else dv(dev, rs), B, C, T, y.ptr())
        gy = y.read().reshape(B, C, T)
        assert y.stray() == 0
        ry = G.prelu_res_fwd(act, sl, rs)
        if rs is None:
            assert np.array_equal(bits(gy), bits(ry.astype(f32)))           # a or slope a: at most one rounding, -0 kept
        # slope a + res: k = 2
        assert ratio(gy, ry, 2 * U * (np.abs(act.astype(f64)) + (0 if rs is None else np.abs(rs.astype(f64))))) <= tol
    da, part = Buf(dev, z.size), Buf(dev, B * C)
    call("mx_prelu_res_bwd", dv(dev, gr), dv(dev, act), dv(dev, slope), B, C, T, da.ptr(), part.ptr())
    gda, gpart = da.read().reshape(B, C, T), part.read()
    assert da.stray() == 0 and part.stray() == 0
    rda, rpart, mag = G.prelu_res_bwd(gr, act, slope)
    assert np.array_equal(bits(gda), bits(rda.astype(f32)))                 # at +0 and -0: slope dy
    assert ratio(gpart, rpart, fp64_once(rpart, mag)) <= tol


# ==== the generic LSTM recurrence ==============================================================================================
R_LSTM = 8.0


def _extend(p):
    """The same problem with one more hidden unit whose weights, biases, inputs, state and gradient are all zero: the shared
    units compute the same sums in the same order (the extra terms are exact zeros)."""
    Hn, B, T = p["Hn"], p["B"], p["T"]

    def gates(a):                                                       # (..., 4 Hn) -> (..., 4 (Hn + 1))
        a4 = a.reshape(a.shape[:-1] + (4, Hn))
        return np.concatenate([a4, np.zeros(a4.shape[:-1] + (1,), f32)], -1).reshape(a.shape[:-1] + (4 * (Hn + 1),))

    def units(a):
        return np.concatenate([a, np.zeros(a.shape[:-1] + (1,), f32)], -1)

    w = np.zeros((4, Hn + 1, Hn + 1), f32)
    w[:, :Hn, :Hn] = p["w_hh"].reshape(4, Hn, Hn)
    return dict(Hn=Hn + 1, B=B, T=T, zin=gates(p["zin"]), b_ih=gates(p["b_ih"]), b_hh=gates(p["b_hh"]), w_hh=w.reshape(4 * (Hn + 1), Hn + 1),
                h0=units(p["h0"]), c0=units(p["c0"]), dhfc=units(p["dhfc"]))


@functools.lru_cache(maxsize=None)
def _lstm_problem(Hn, T, extended=False):
    """Inputs on nn.LSTM's init scale + the fp64 and fp32 reference runs, computed once and shared (read only)."""
    if extended:
        p = _extend(_lstm_problem(Hn - 1, T))
    else:
        g = np.random.default_rng(Hn * 100 + T)
        B, D, k = 2, 3, 1 / np.sqrt(Hn)
        un = lambda *s: g.uniform(-k, k, s).astype(f32)
        zin = (g.standard_normal((B, T, D)) @ g.uniform(-k, k, (D, 4 * Hn))).astype(f32)
        p = dict(Hn=Hn, B=B, T=T, zin=zin, b_ih=un(4 * Hn), b_hh=un(4 * Hn), w_hh=un(4 * Hn, Hn), h0=rnd(g, (B, Hn), 0.5),
                 c0=rnd(g, (B, Hn), 0.5), dhfc=rnd(g, (B, T, Hn)))
    fw = (p["zin"], p["b_ih"], p["b_hh"], p["w_hh"], p["h0"], p["c0"])
    p["fwd64"], p["fwd32"] = G.lstmg_fwd(*fw), G.lstmg_fwd(*fw, dtype=f32)
    p["stash_in"] = p["fwd64"][0].astype(f32)                             # the backward kernel's input: independent of the forward kernel
    bw = (p["stash_in"], p["dhfc"], p["w_hh"], p["c0"])
    p["bwd64"], p["bwd32"] = G.lstmg_bwd(*bw), G.lstmg_bwd(*bw, dtype=f32)
    for v in p.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return p


def _lstm_run(dev, p):
    B, T, Hn = p["B"], p["T"], p["Hn"]
    stash, h1, c1, dgate = Buf(dev, B * T * 6 * Hn), Buf(dev, B * Hn), Buf(dev, B * Hn), Buf(dev, B * T * 4 * Hn)
    call("mx_lstmg_fwd", dv(dev, p["zin"]), dv(dev, p["b_ih"]), dv(dev, p["b_hh"]), dv(dev, p["w_hh"]), dv(dev, p["h0"]), dv(dev, p["c0"]),
         B, T, Hn, stash.ptr(), h1.ptr(), c1.ptr())
    call("mx_lstmg_bwd", dv(dev, p["stash_in"]), dv(dev, p["dhfc"]), dv(dev, p["w_hh"]), dv(dev, p["c0"]), B, T, Hn, dgate.ptr())
    got = dict(stash=stash.read().reshape(B, T, 6, Hn), h1=h1.read().reshape(B, Hn), c1=c1.read().reshape(B, Hn),
               dgate=dgate.read().reshape(B, T, 4 * Hn))
    assert stash.stray() == 0 and h1.stray() == 0 and c1.stray() == 0 and dgate.stray() == 0
    return got


def _lstm_gate(p, got):
    """err <= R max(e32, u max|ref|) per tensor; returns {tensor: err / max(e32, floor)}."""
    s64, h64, c64 = p["fwd64"]
    s32, h32, c32 = p["fwd32"]
    tens = {name: (got["stash"][:, :, q], s64[:, :, q], s32[:, :, q]) for q, name in enumerate("ifgoch")}
    tens.update(h1=(got["h1"], h64, h32), c1=(got["c1"], c64, c32), dgate=(got["dgate"], p["bwd64"], p["bwd32"]))
    out = {}
    for name, (g_, r64, r32) in tens.items():
        err, e32 = float(np.abs(g_.astype(f64) - r64).max()), float(np.abs(r32.astype(f64) - r64).max())
        out[name] = err / max(e32, U * float(np.abs(r64).max()), 1e-300)
        assert np.isfinite(g_).all(), name
    return out


@pytest.mark.parametrize("Hn,T", [(1, 24), (7, 24), (62, 24), (63, 24), (96, 24), (97, 24), (257, 24), (97, 1)])
def test_lstmg_recurrence(dev, Hn, T):
    """The whole stash (i, f, g, o, c, h of every step), h1, c1 and dgate against the fp64 recurrence, non-zero h0 / c0, B = 2.
    62 | 63: the dynamic-LDS attribute (64 KB); 96 | 97: W_hh in LDS | in global memory (150 KB); 257: every per-thread loop
    strides more than once.  Gate: err <= R max(e32, u max|ref|) with R = 8.

    Measured on the MI355X, err / max(e32, floor), worst tensor of each (Hn, T):
        (1, 24) 1.32 h | (7, 24) 1.25 c | (62, 24) 2.35 g | (63, 24) 2.07 g | (96, 24) 3.36 c1 | (97, 24) 2.63 g |
        (257, 24) 3.41 c1 | (97, 1) 2.51 g;  dgate <= 1.00 everywhere.
    Twice the worst (3.41) rounded up to a power of two: R = 8.  The kernel's expf / tanhf and its sequential fused
    multiply-adds cost a small factor over numpy's fp32 run of the same formulae (whose dot products are blocked), not an
    order of magnitude."""
    p = _lstm_problem(Hn, T)
    ratios = _lstm_gate(p, _lstm_run(dev, p))
    print("lstmg ratios", Hn, T, {k: round(v, 3) for k, v in ratios.items()})
    tol = R_LSTM
    for name, r in ratios.items():
        assert r <= tol, (name, ratios)


@pytest.mark.parametrize("Hn", [62, 96])
def test_lstmg_path_switch_is_bit_identical(dev, Hn):
    """Hn and Hn + 1 sit on either side of a path switch (62 | 63 the LDS attribute, 96 | 97 W_hh in LDS | global).  The Hn + 1
    problem is the Hn one with a zero-weighted extra unit, so both paths run the same arithmetic in the same order on the shared
    units: both pass the yardstick gate, and the shared units agree bit for bit."""
    small, big = _lstm_problem(Hn, 24), _lstm_problem(Hn + 1, 24, True)
    gs, gb = _lstm_run(dev, small), _lstm_run(dev, big)
    tol = R_LSTM
    for p, got in ((small, gs), (big, gb)):
        for name, r in _lstm_gate(p, got).items():
            assert r <= tol, (p["Hn"], name)
    B, T = 2, 24
    assert np.array_equal(bits(gb["stash"][..., :Hn]), bits(gs["stash"]))
    assert np.array_equal(bits(gb["h1"][:, :Hn]), bits(gs["h1"])) and np.array_equal(bits(gb["c1"][:, :Hn]), bits(gs["c1"]))
    assert np.array_equal(bits(gb["dgate"].reshape(B, T, 4, Hn + 1)[..., :Hn]), bits(gs["dgate"].reshape(B, T, 4, Hn)))
    assert not gb["stash"][:, :, 5, Hn].any() and not gb["dgate"].reshape(B, T, 4, Hn + 1)[..., Hn].any()


@pytest.mark.parametrize("T", [1, 257])
@pytest.mark.parametrize("in_ch,out_ch", [(1, 1), (2, 2), (1, 3), (3, 1)])
def test_lstmg_out_fwd_bwd(dev, T, in_ch, out_ch):
    g = np.random.default_rng(T + in_ch * 4 + out_ch)
    B, Co = 2, max(in_ch, out_ch)
    fc, bias, x = g.uniform(-0.8, 0.8, (B, T, out_ch)).astype(f32), g.uniform(-0.2, 0.2, out_ch).astype(f32), g.uniform(-1, 1, (B, in_ch, T)).astype(f32)
    y = Buf(dev, B * Co * T)
    call("mx_lstmg_out_fwd", dv(dev, fc), dv(dev, bias), dv(dev, x), B, T, out_ch, in_ch, y.ptr())
    gy = y.read().reshape(B, Co, T)
    assert y.stray() == 0
    tol = 1.0
    # |fc + bias| <= 1, |.. + x| <= 2: the two additions round by <= 2 (u / 2) 2 = 2 u, tanh's slope is <= 1, tanhf <= 2 u: 4 ulp of 1
    assert ratio(gy, G.lstmg_out_fwd(fc, bias, x), 4 * U) <= tol
    dy = rnd(g, (B, Co, T))
    dpre = Buf(dev, B * T * out_ch)
    call("mx_lstmg_out_bwd", dv(dev, dy), dv(dev, gy), B, T, out_ch, Co, dpre.ptr())
    gd = dpre.read().reshape(B, T, out_ch)
    assert dpre.stray() == 0
    mag = np.abs(dy.astype(f64)) * (1 + gy.astype(f64) ** 2)
    if out_ch != Co:
        mag = mag.sum(1, keepdims=True)
    # dy (1 - y y): multiply, subtract, multiply, then Co - 1 additions over the broadcast channels: k = 3 + Co - 1
    assert ratio(gd, G.lstmg_out_bwd(dy, gy, out_ch), (2 + Co) * U * mag.transpose(0, 2, 1)) <= tol


# ==== argument checks: the documented status, before any launch =================================================================
def _arg_cases():
    X = "X"                                                             # a valid device pointer
    ok = {
        "mx_sgemm_f32": [X, 4, 1, 0, X, 4, 1, 0, X, 4, 1, 0, 4, 4, 4, 1, 1, 0],
        "mx_tcn_im2col": [X, X, 2, 2, 8, 8, 3, 1, 1, X],
        "mx_tcn_col2im": [X, 2, 2, 8, 8, 3, 1, 1, X],
        "mx_tcn_act_fwd": [X, X, X, X, 2, 2, 8, X],
        "mx_tcn_act_bwd": [X, X, X, 2, 2, 8, X, X],
        "mx_tcn_ln_bwd": [X, X, X, X, 2, 2, 8, X],
        "mx_im2col2d": [X, 2, 2, 4, 4, 3, 3, 1, 1, 1, 1, X],
        "mx_col2im2d": [X, 2, 2, 4, 4, 3, 3, 1, 1, 1, 1, X],
        "mx_rowln_fwd": [X, 2, 8, 1e-5, X, X],
        "mx_rowln_bwd": [X, X, X, 2, 8, X],
        "mx_row_sums": [X, 2, 8, X],
        "mx_pool_prelu_fwd": [X, X, 4, 2, 4, 4, 2, X, X, X, X],
        "mx_pool_prelu_bwd": [X, X, X, 4, 2, 4, 4, 2, X, X, X],
        "mx_binmean_head_fwd": [X, 2, 2, 4, 4, X, X, 2, X, X],
        "mx_binmean_head_bwd": [X, X, X, X, 2, 2, 4, 4, 2, X, X],
        "mx_lstmg_fwd": [X, X, X, X, X, X, 2, 3, 4, X, X, X],
        "mx_lstmg_bwd": [X, X, X, X, 2, 3, 4, X],
        "mx_lstmg_out_fwd": [X, X, X, 2, 4, 2, 2, X],
        "mx_lstmg_out_bwd": [X, X, 2, 4, 2, 2, X],
        "mx_chan_stats": [X, 2, 2, 8, X],
        "mx_chan_norm_fwd": [X, X, 2, 2, 8, X],
        "mx_chan_norm_bwd": [X, X, X, 2, 2, 8, 1, X],
        "mx_film_fwd": [X, X, 2, 2, 8, X],
        "mx_film_bwd": [X, X, X, 2, 2, 8, X, X],
        "mx_prelu_res_fwd": [X, X, X, 2, 2, 8, X],
        "mx_prelu_res_bwd": [X, X, X, 2, 2, 8, X, X],
    }
    ARG, UNS = -1, -2
    bad = [  # (entry point, index of the argument, its bad value, status)
        ("mx_sgemm_f32", 0, None, ARG), ("mx_sgemm_f32", 4, None, ARG), ("mx_sgemm_f32", 8, None, ARG), ("mx_sgemm_f32", 12, 0, ARG),
        ("mx_sgemm_f32", 13, -1, ARG), ("mx_sgemm_f32", 14, 0, ARG), ("mx_sgemm_f32", 15, 0, ARG), ("mx_sgemm_f32", 16, 0, ARG),
        ("mx_tcn_im2col", 0, None, ARG), ("mx_tcn_im2col", 9, None, ARG), ("mx_tcn_im2col", 4, 353, ARG), ("mx_tcn_im2col", 6, 0, ARG),
        ("mx_tcn_im2col", 8, 0, ARG), ("mx_tcn_col2im", 8, None, ARG), ("mx_tcn_col2im", 3, 353, ARG), ("mx_tcn_col2im", 7, 0, ARG),
        ("mx_tcn_col2im", 1, -2, ARG),
        ("mx_tcn_act_fwd", 0, None, ARG), ("mx_tcn_act_fwd", 7, None, ARG), ("mx_tcn_act_fwd", 6, 353, ARG), ("mx_tcn_act_fwd", 4, 0, ARG),
        ("mx_tcn_act_bwd", 7, None, ARG), ("mx_tcn_act_bwd", 5, 0, ARG), ("mx_tcn_ln_bwd", 2, None, ARG), ("mx_tcn_ln_bwd", 6, 353, ARG),
        ("mx_im2col2d", 11, None, ARG), ("mx_im2col2d", 5, 0, ARG), ("mx_im2col2d", 9, -1, ARG), ("mx_col2im2d", 0, None, ARG),
        ("mx_col2im2d", 4, 0, ARG), ("mx_col2im2d", 7, 0, ARG),
        ("mx_rowln_fwd", 5, None, ARG), ("mx_rowln_fwd", 2, 0, ARG), ("mx_rowln_bwd", 5, None, ARG), ("mx_rowln_bwd", 3, -1, ARG),
        ("mx_row_sums", 3, None, ARG), ("mx_row_sums", 2, 0, ARG),
        ("mx_pool_prelu_fwd", 10, None, ARG), ("mx_pool_prelu_fwd", 6, 0, ARG), ("mx_pool_prelu_fwd", 6, 5, UNS),
        ("mx_pool_prelu_fwd", 3, 3, UNS), ("mx_pool_prelu_bwd", 8, None, ARG), ("mx_pool_prelu_bwd", 7, 5, UNS),
        ("mx_pool_prelu_bwd", 4, 3, UNS), ("mx_pool_prelu_bwd", 3, 0, ARG),
        ("mx_binmean_head_fwd", 6, None, ARG), ("mx_binmean_head_fwd", 7, 0, ARG), ("mx_binmean_head_bwd", 9, None, ARG),
        ("mx_binmean_head_bwd", 6, 0, ARG),
        ("mx_lstmg_fwd", 10, None, ARG), ("mx_lstmg_fwd", 8, 0, ARG), ("mx_lstmg_fwd", 7, 0, ARG), ("mx_lstmg_fwd", 8, 4097, UNS),
        ("mx_lstmg_bwd", 7, None, ARG), ("mx_lstmg_bwd", 4, 0, ARG), ("mx_lstmg_bwd", 6, -3, ARG),
        ("mx_lstmg_out_fwd", 7, None, ARG), ("mx_lstmg_out_fwd", 4, 0, ARG),
        ("mx_lstmg_out_bwd", 6, None, ARG), ("mx_lstmg_out_bwd", 5, 3, ARG),
        ("mx_chan_stats", 4, None, ARG), ("mx_chan_stats", 3, 0, ARG), ("mx_chan_norm_fwd", 1, None, ARG), ("mx_chan_norm_bwd", 7, None, ARG),
        ("mx_chan_norm_bwd", 4, 0, ARG), ("mx_film_fwd", 1, None, ARG), ("mx_film_bwd", 7, None, ARG), ("mx_film_bwd", 3, -1, ARG),
        ("mx_prelu_res_fwd", 6, None, ARG), ("mx_prelu_res_fwd", 3, -1, ARG), ("mx_prelu_res_bwd", 2, None, ARG), ("mx_prelu_res_bwd", 7, None, ARG),
    ]
    return ok, bad + [("mx_lstmg_out_fwd", (5, 6), (2, 3), ARG)]       # (out_ch, in_ch) = (2, 3)


def test_argument_checks_return_the_documented_status(dev):
    """One argument of an otherwise valid call is made invalid: NULL, a zero or negative size, T = 353, batches_per_group = 0,
    a pool taller than the image, planes % C != 0, (out_ch, in_ch) = (2, 3).  The status must come back without a launch.  (The
    valid pointer is a zeroed 4 MB buffer, far larger than anything these sizes address.)"""
    ok, bad = _arg_cases()
    big = torch.zeros(1 << 20, device=dev)
    before = big.clone()
    for name, idx, val, want in bad:
        args = list(ok[name])
        for i, v in zip(idx if isinstance(idx, tuple) else (idx,), val if isinstance(val, tuple) else (val,)):
            args[i] = v
        args = [big if isinstance(a, str) else a for a in args]
        assert status(name, *args) == want, (name, idx, val)
    torch.cuda.synchronize()
    assert torch.equal(big, before)

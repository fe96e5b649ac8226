"""GPU: the warp (K26, csrc/warp.hip) against its fp64 restatement, tests/helpers/warp64.py, on the kernel's own inputs.

The gate is the header's, derived and not chosen:  |y - y64| <= 2^-24 |y64| + T 2^-53 sum |h x| + 2^-40 sum |x|  over the
taps' samples -- one fp32 rounding, the fp64 sums of T products on either side, and the 2^-40 a tap that K24's tap gate
grants (the kernel's taps come by angle addition and a reciprocal table).  An output whose window misses the row has a gate
of zero: it must be an exact zero.  The worst fraction of the gate used is printed.

n_out = 1, 5 and OUT_TILE - 1, OUT_TILE, OUT_TILE + 1, 2 OUT_TILE + 8 (the tile is 1024, not K24's 4096: straddled the same
way); n_in differs from n_out; drift in {0, +-2e-4, +-1e-3}; offset in {0, 0.5, -3.25, 37.4, one that reads past the row's
end, one that starts before sample 0}; B = 1 and 3 with other parameters in every row; row strides n and n + 1; x, y, offset,
drift and sign each at another offset from a 16-byte boundary; amplitudes 1 and 1e-4."""
import numpy as np
import pytest
import torch

from tests.helpers import warp64 as h
from tests.test_gpu_resample import SENTINEL, strided

pytestmark = pytest.mark.gpu

T = h.plan()[1]
DRIFTS = (0.0, 2e-4, -2e-4, 1e-3, -1e-3)
N_OUTS = (1, 5, h.OUT_TILE - 1, h.OUT_TILE, h.OUT_TILE + 1, 2 * h.OUT_TILE + 8)


def offsets(n_in):
    return (0.0, 0.5, -3.25, 37.4, n_in - 20.25, -70.5)


def off_boundary(dev, a, dtype, lead):
    """``a`` on the device, ``lead`` elements after a 16-byte boundary."""
    buf = torch.zeros(len(a) + lead, device=dev, dtype=dtype)
    assert buf.data_ptr() % 16 == 0
    buf[lead:] = torch.as_tensor(np.asarray(a), dtype=dtype)
    return buf[lead:]


def run(dev, x, offset, drift, sign, n_out, x_extra, xo, yo, y_extra, lead):
    """warp_rows on a strided x into a strided out; returns y (numpy) after checking that no other float moved."""
    from mod_extraction_amd import alignment
    B, n = x.shape
    xv, _ = strided(dev, x, n + x_extra, xo)
    yv, ybuf = strided(dev, (B, n_out), n_out + y_extra, yo, fill=SENTINEL)
    got = alignment.warp_rows(xv, off_boundary(dev, offset, torch.float64, lead % 2), off_boundary(dev, drift, torch.float64, (lead + 1) % 2),
                              n_out=n_out, polarity=None if sign is None else off_boundary(dev, sign, torch.float32, 1 + lead % 3),
                              out=yv)
    assert got.data_ptr() == yv.data_ptr()
    y = yv.cpu().numpy()
    rest = ybuf.clone()
    rest[yo:].as_strided((B, n_out), (n_out + y_extra, 1)).fill_(SENTINEL)
    assert bool((rest == SENTINEL).all()), "a float outside the rows of out was written"
    return y


def used(y, x, offset, drift, sign, n_out):
    """(worst fraction of the gate used, number of outputs whose window misses the row -- those must be exact zeros)"""
    y64, a, ax = h.rows(x, offset, drift, n_out=n_out, sign=sign, with_bound=True)
    tol = h.gate(y64, a, ax, T)
    err = np.abs(y.astype(np.float64) - y64)
    outside = ax == 0.0
    assert y.shape == y64.shape and not np.isnan(y).any()
    assert np.all(y[outside] == 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(err == 0.0, 0.0, err / tol)
    return float(frac.max()), int(outside.sum())


def test_rows_against_the_helper(dev):
    r = np.random.default_rng(26)
    worst, zeros_seen, i = 0.0, 0, 0
    for n_out in N_OUTS:
        for B in (1, 3):
            n_in = n_out + (7, -3, 130)[i % 3] if n_out > 5 else n_out + 2 + i
            amp = (1.0, 1e-4)[(i // 2) % 2]
            x = (amp * r.standard_normal((B, n_in))).astype(np.float32)
            drift = np.array([DRIFTS[(i + 2 * b) % 5] for b in range(B)])
            offset = np.array([offsets(n_in)[(i + b) % 6] for b in range(B)])
            sign = None if i % 3 == 0 else np.array([(-1.0, 0.7, -0.0)[(i + b) % 3] for b in range(B)], dtype=np.float32)
            xo, yo = (int(v) for v in r.integers(0, 4, 2))
            y = run(dev, x, offset, drift, sign, n_out, i % 2, xo, yo, (i // 2) % 2, i)
            f, z = used(y, x, offset, drift, sign, n_out)
            print(f"case {i}: n {n_in} -> {n_out}, B {B}, drift {drift.tolist()}, offset {offset.tolist()}: {f:.3f} of the gate, {z} zeros")
            worst, zeros_seen, i = max(worst, f), zeros_seen + z, i + 1
    print(f"worst fraction of the gate used: {worst:.3f}")
    assert i == 12 and zeros_seen > 0
    assert worst <= 1.0


def test_every_drift_and_offset(dev):
    """All 30 (drift, offset) pairs as the rows of ONE launch, a tile and one output long."""
    n_out, n_in = h.OUT_TILE + 1, h.OUT_TILE + 40
    x = np.random.default_rng(27).standard_normal((30, n_in)).astype(np.float32)
    drift = np.repeat(DRIFTS, 6)
    offset = np.tile(offsets(n_in), 5)
    y = run(dev, x, offset, drift, None, n_out, 1, 3, 1, 0, 1)
    f, z = used(y, x, offset, drift, None, n_out)
    print(f"30 rows: {f:.3f} of the gate, {z} exact zeros")
    assert z > 0
    assert f <= 1.0


def test_polarity_scaling_determinism_and_views(dev):
    from mod_extraction_amd import alignment
    n_in, n_out = 2 * h.OUT_TILE + 77, 2 * h.OUT_TILE + 5
    x = torch.from_numpy(np.random.default_rng(28).standard_normal((3, n_in)).astype(np.float32)).to(dev)
    off = torch.tensor([37.4, -3.25, 0.5], device=dev, dtype=torch.float64)
    dr = torch.tensor([2e-4, -1e-3, 0.0], device=dev, dtype=torch.float64)
    y = alignment.warp_rows(x, off, dr, n_out=n_out)
    assert y.shape == (3, n_out) and y.is_contiguous()
    assert torch.equal(alignment.warp_rows(x, off, dr, n_out=n_out), y)                              # the same bits again
    assert torch.equal(alignment.warp_rows(0.25 * x, off, dr, n_out=n_out), 0.25 * y)                # a power of two passes through
    neg = alignment.warp_rows(x, off, dr, n_out=n_out, polarity=-1)
    assert torch.equal(neg.view(torch.int32), y.view(torch.int32) ^ torch.tensor(-2 ** 31, dtype=torch.int32, device=dev))
    mixed = alignment.warp_rows(x, off, dr, n_out=n_out, polarity=torch.tensor([-0.3, 0.9, -1.0], device=dev))
    assert torch.equal(mixed[0], neg[0]) and torch.equal(mixed[1], y[1]) and torch.equal(mixed[2], neg[2])
    assert torch.equal(alignment.warp_rows(x[1], -3.25, -1e-3, n_out=n_out), y[1])                   # a row alone, float parameters
    assert alignment.warp_rows(x[0], 0.0, 0.0).shape == (n_in,)                                     # n_out defaults to n
    wide = torch.full((3, n_out + 9), SENTINEL, device=dev)
    got = alignment.warp_rows(x, off, dr, n_out=n_out, out=wide[:, 4:4 + n_out])
    assert torch.equal(got, y) and bool((wide[:, :4] == SENTINEL).all()) and bool((wide[:, 4 + n_out:] == SENTINEL).all())
    # device parameters beyond the limits cannot be refused without a synchronisation: the row is NaN, its neighbours are not
    bad = alignment.warp_rows(x, off, torch.tensor([2e-4, 2e-3, float("nan")], device=dev, dtype=torch.float64), n_out=n_out)
    assert torch.equal(bad[0], y[0]) and bool(torch.isnan(bad[1:]).all())
    with pytest.raises(ValueError, match="limits"):
        alignment.warp_rows(x, 0.0, 2e-3)
    with pytest.raises(ValueError, match="overlap"):
        alignment.warp_rows(x, off, dr, out=x)


def test_uninitialised_memory_changes_no_bit(dev):
    from mod_extraction_amd import alignment
    from tests.test_gpu_uninit_independence import _dv, _rng, run_patterns
    n = h.OUT_TILE + 3
    wide = _dv(dev, _rng(n).standard_normal((3, n + 5)))
    x = wide[:, 2:2 + n]                                        # rows a stride apart, off the 16-byte boundary

    def case():
        return {"y": alignment.warp_rows(x, 37.4, 3e-4, n_out=n + 50, polarity=-1),
                "short": alignment.warp_rows(x[:, :3], -0.5, 0.0, n_out=200)}       # every output is all edge

    run_patterns(case, {"alignment:warp_rows"})

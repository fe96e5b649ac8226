"""Philox-4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) in numpy uint64 arithmetic,
vectorised over the counter, and the mapping of csrc/noise.hip (mx_uniform_rows) from its words to a row of uniform samples.

One round, on the counter (c0, c1, c2, c3) with the key (k0, k1):
    (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0)),   M0 = 0xD2511F53, M1 = 0xCD9E8D57,
and the key moves by (0x9E3779B9, 0xBB67AE85) after every round; ten rounds.

``uniform_row``: sample j of clip ``clip`` in batch ``counter`` of the stream ``seed`` is word j % 4 of the block with the counter
(j / 4, clip, counter, 0x6d6f6478) under the key (seed & 0xffffffff, seed >> 32); with u = word >> 8 (24 bits) and
s = fl32(fl32(hi - lo) 2^-24) the value is fmaf(u, s, lo): ONE rounding of u s + lo.  Here it is fl32(f64(u) f64(s) + f64(lo)),
which is the same number whenever the fp64 sum is exact: u s has at most 48 significant bits below 2^(e + 1), e the exponent of
hi - lo, and lo has 24 below 2^(e' + 1); when |e - e'| <= 4 the two fit into 52 bits together (or lo is 0), so fp64 holds the sum
exactly and the only rounding is the one to fp32.  Anything else raises.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
TAG = 0x6d6f6478                                      # the fourth counter word of csrc/noise.hip
MASK = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: (..., 4) integers below 2^32, key: two integers below 2^32 -> (..., 4) uint32."""
    c = np.asarray(counter, np.uint64)
    assert c.shape[-1] == 4 and int(c.max(initial=0)) <= 0xFFFFFFFF
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = int(key[0]), int(key[1])
    assert 0 <= k0 <= 0xFFFFFFFF and 0 <= k1 <= 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                            # 32 x 32 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> _32) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def _exact_in_f64(lo, span):
    if lo == 0.0:
        return True
    return abs(int(np.frexp(np.float64(lo))[1]) - int(np.frexp(np.float64(span))[1])) <= 4


def row_words(seed, counter, clip, n):
    """The first n 32-bit words of the stream (seed, counter, clip)."""
    seed, counter, clip, n = int(seed), int(counter), int(clip), int(n)
    assert 0 <= seed < 1 << 64 and 0 <= counter <= 0xFFFFFFFF and 0 <= clip <= 0xFFFFFFFF and n >= 0
    j4 = np.arange((n + 3) // 4, dtype=np.uint64)
    ctr = np.stack([j4, np.full_like(j4, clip), np.full_like(j4, counter), np.full_like(j4, TAG)], -1)
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:n]


def uniform_row(seed, counter, clip, n, lo, hi):
    """(n,) float32: what mx_uniform_rows writes for clip ``clip`` with (seed, counter, lo, hi)."""
    lo32, hi32 = np.float32(lo), np.float32(hi)
    assert hi32 > lo32
    span = np.float32(hi32 - lo32)
    s = np.float32(span * np.float32(2.0 ** -24))
    if not _exact_in_f64(float(lo32), float(span)):
        raise ValueError(f"uniform_row: u s + lo is not exact in fp64 for lo = {lo32}, hi - lo = {span}")
    u = (row_words(seed, counter, clip, n) >> np.uint32(8)).astype(np.float64)
    return (u * np.float64(s) + np.float64(lo32)).astype(np.float32)

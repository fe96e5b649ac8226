"""CPU: the numpy Philox-4x32-10 of tests/helpers/philox_ref.py against the published known-answer vectors, the layout properties
of ``uniform_row`` that tests/test_gpu_noise_units.py relies on, and the statistics of the stream the batcher requests."""
import itertools

import numpy as np
import pytest
import torch

from tests.helpers import philox_ref as P

# the kat_vectors of the Random123 distribution for philox4x32, 10 rounds: counter, key, output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def _peak():
    from mod_extraction_amd import data_modules
    return data_modules.SyntheticFxBatcher(1, 4410, 44100, ("flanger",), torch.device("cpu")).peak


def _ranges():
    p = _peak()
    return [(-p, p), (-1.0, 1.0), (0.0, 1.0), (0.25, 0.75)]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_known_answers(ctr, key, want):
    got = P.philox4x32_10(np.array(ctr, np.uint64), key)
    assert got.dtype == np.uint32 and [int(v) for v in got] == list(want)


def test_vectorised_over_the_counter():
    """A stack of counters gives the stack of the single results (the third vector's key, the three counters)."""
    ctr = np.array([k[0] for k in KAT], np.uint64)
    got = P.philox4x32_10(ctr, KAT[2][1])
    for i in range(3):
        assert np.array_equal(got[i], P.philox4x32_10(ctr[i], KAT[2][1]))
    assert [int(v) for v in got[2]] == list(KAT[2][2])
    assert np.array_equal(P.philox4x32_10(ctr.reshape(3, 1, 4), KAT[2][1])[:, 0], got)


def test_a_row_is_the_head_of_a_longer_one():
    long = P.uniform_row(43, 1, 2, 4099, -1.0, 1.0)
    for n in (0, 1, 3, 4, 5, 1023, 1024, 1025):
        assert np.array_equal(P.uniform_row(43, 1, 2, n, -1.0, 1.0).view(np.int32), long[:n].view(np.int32)), n
    assert P.uniform_row(43, 1, 2, 0, -1.0, 1.0).shape == (0,)


def test_the_words_of_a_row():
    """Sample j is word j % 4 of the block (j / 4, clip, counter, tag) under the key (seed low, seed high)."""
    seed, counter, clip = (7 << 32) + 43, 9, 5
    w = P.row_words(seed, counter, clip, 11)
    for j in range(11):
        blk = P.philox4x32_10(np.array([j // 4, clip, counter, 0x6d6f6478], np.uint64), (43, 7))
        assert int(w[j]) == int(blk[j % 4])
    v = P.uniform_row(seed, counter, clip, 11, 0.0, 1.0)
    assert np.array_equal(v, ((w >> 8).astype(np.float64) * 2.0 ** -24).astype(np.float32))       # (0, 1): exact in fp32


def test_every_part_of_the_stream_address_matters():
    base = dict(seed=43, counter=1, clip=0)
    ref = P.uniform_row(n=64, lo=-1.0, hi=1.0, **base)
    others = [dict(base, seed=44), dict(base, seed=43 + (1 << 32)), dict(base, seed=43 + (1 << 63)), dict(base, counter=2),
              dict(base, counter=0xFFFFFFFF), dict(base, clip=1), dict(base, clip=65534)]
    rows = [ref] + [P.uniform_row(n=64, lo=-1.0, hi=1.0, **o) for o in others]
    for a, b in itertools.combinations(rows, 2):
        assert not np.array_equal(a, b)
        assert not (a == b).any()                   # 24-bit values: a coincidence in 64 samples has probability 4e-6


def test_values_lie_in_the_half_open_range():
    for lo, hi in _ranges():
        lo32, hi32 = np.float32(lo), np.float32(hi)
        for clip in range(4):
            v = P.uniform_row(43, 1, clip, 4099, lo, hi)
            assert v.dtype == np.float32 and (v >= lo32).all() and (v < hi32).all(), (lo, hi)
            assert v.min() < lo32 + 0.01 * (hi32 - lo32) and v.max() > hi32 - 0.01 * (hi32 - lo32)       # and fill it


def test_inexact_ranges_raise():
    with pytest.raises(ValueError):
        P.uniform_row(43, 1, 0, 4, 1.0e-3, 1.0)      # exponents 10 apart: u s + lo needs more than 53 bits
    with pytest.raises(ValueError):
        P.uniform_row(43, 1, 0, 4, -100.0, -99.0)
    P.uniform_row(43, 1, 0, 4, 0.0, 1.0e-3)          # lo == 0: always exact
    P.uniform_row(43, 1, 0, 4, 1.0 / 16, 1.0)        # 4 apart


def test_the_stream_the_batcher_requests_looks_uniform():
    """seed 43 (the batcher's default audio_seed), counter 1 (its first batch), clips 0 .. 3, 4096 samples on (0, 1): mean,
    variance, lag-1 autocorrelation and every cross-clip correlation within 6 standard errors of an ideal U(0, 1) stream of
    that length (sd 0.2887; mean: sd / 64; variance of U(0, 1) = 1 / 12 with standard error sqrt(1 / 180) / 64; a sample
    correlation of independent streams: 1 / 64)."""
    n = 4096
    x = np.stack([P.uniform_row(43, 1, c, n, 0.0, 1.0) for c in range(4)]).astype(np.float64)
    root = np.sqrt(n)
    mean, var = x.mean(1), x.var(1)
    print("[measured] philox stream: worst |mean - 1/2|", float(np.abs(mean - 0.5).max()), "worst |var - 1/12|",
          float(np.abs(var - 1 / 12).max()))
    assert (np.abs(mean - 0.5) <= 6 * 0.2887 / root).all(), mean
    assert (np.abs(var - 1.0 / 12.0) <= 6 * np.sqrt(1.0 / 180.0) / root).all(), var
    z = (x - mean[:, None]) / x.std(1)[:, None]
    lag1 = (z[:, 1:] * z[:, :-1]).mean(1)
    cross = np.array([(z[a] * z[b]).mean() for a, b in itertools.combinations(range(4), 2)])
    print("[measured] philox stream: worst lag-1", float(np.abs(lag1).max()), "worst cross-clip", float(np.abs(cross).max()))
    assert (np.abs(lag1) <= 6 / root).all(), lag1
    assert (np.abs(cross) <= 6 / root).all(), cross

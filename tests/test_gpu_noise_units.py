"""GPU: mx_uniform_rows (csrc/noise.hip), the Philox-4x32-10 stream behind every sample of synthetic dry audio, on its raw entry
point and through SyntheticFxBatcher, against tests/helpers/philox_ref.py.  Every comparison is on bits.

Conventions of tests/test_gpu_midblock_units.py: the output is an ``Out`` between two guard bands, body and guards pre-filled with
a NaN bit pattern; the WHOLE body is compared with an image that holds the reference row where a sample is in range and the
sentinel everywhere else (the tail of a row up to its stride, unlisted rows, the wet half of a dry / wet pair), the number of
sentinel words left is counted, and both guard bands must be intact.
"""
import numpy as np
import pytest
import torch

from tests.helpers import philox_ref as P
from tests.helpers.gpu_harness import ARG, SENT, UNSUPPORTED, Out, call, dv, status

pytestmark = pytest.mark.gpu
LENGTHS = [1, 3, 4, 5, 1023, 1024, 1025, 4099]      # float4 groups, the scalar tail, the 1024-sample grid boundary
SEEDS = [43, (1 << 32) + 43, (1 << 63) + 1]
COUNTERS = [1, 2, 0xFFFFFFFF]


def _peak():
    from mod_extraction_amd import data_modules
    return data_modules.SyntheticFxBatcher(1, 4410, 44100, ("flanger",), torch.device("cpu")).peak


def _ranges():
    p = _peak()
    return [(-p, p), (-1.0, 1.0), (0.0, 1.0), (0.25, 0.75)]


def _image(n_clips, stride, rows, lens, len_add, seed, counter, lo, hi):
    """The expected body, as int32 words: row ``clip`` holds uniform_row(...) on its first lens[clip] + len_add samples for every
    listed clip, the sentinel everywhere else.  Also the number of samples written."""
    img = np.full(n_clips * stride, SENT, np.int32)
    written = 0
    for clip in (range(n_clips) if rows is None else rows):
        n = (0 if lens is None else int(lens[clip])) + len_add
        img[clip * stride:clip * stride + n] = P.uniform_row(seed, counter, clip, n, lo, hi).view(np.int32)
        written += n
    return img, written


def _run(dev, n_clips, stride, rows=None, lens=None, len_add=0, max_len=None, seed=43, counter=1, lo=-1.0, hi=1.0):
    """One launch into a fresh Out of n_clips rows; the body against its image.  Returns the body's words."""
    max_len = len_add if max_len is None else max_len
    out = Out(dev, n_clips * stride)
    rows_d = None if rows is None else dv(dev, np.array(rows, np.int32), np.int32)
    lens_d = None if lens is None else dv(dev, np.array(lens, np.int32), np.int32)
    n_rows = n_clips if rows is None else len(rows)
    call("mx_uniform_rows", out, stride, rows_d, n_rows, lens_d, len_add, max_len, seed, counter, lo, hi)
    img, written = _image(n_clips, stride, rows, lens, len_add, seed, counter, lo, hi)
    body = out.read().view(np.int32)
    assert out.guards_intact()
    assert out.untouched() == out.words - written                  # no generated value is the sentinel (a NaN)
    bad = np.nonzero(body != img)[0]
    assert bad.size == 0, (f"{bad.size} words differ, first at row {bad[0] // stride} sample {bad[0] % stride}: "
                           f"{body[bad[0]]:#x} != {img[bad[0]]:#x}")
    return body


@pytest.mark.parametrize("n", LENGTHS)
def test_rows_at_their_own_stride(dev, n):
    """rows = NULL, lens = NULL, three clips, stride = n .. n + 3: one of the four is a multiple of 4 (vector stores, and a scalar
    tail when n % 4), the other three are the all-scalar path, where rows 1 and 2 start off the 16-byte grid (the phaser staging
    rows of the batcher have such a stride).  Up to three sentinel words between the rows."""
    for stride in range(n, n + 4):
        _run(dev, 3, stride, len_add=n)


@pytest.mark.parametrize("n", LENGTHS)
def test_dry_wet_layout(dev, n):
    """The batch's (B, 2, N) layout: stride = 2 N exactly as SyntheticFxBatcher.render passes it, N a multiple of 4 or not; the
    wet channel right behind every dry row keeps the sentinel (checked by the image)."""
    body = _run(dev, 2, 2 * n, len_add=n, lo=-_peak(), hi=_peak())
    assert (body.reshape(2, 2, n)[:, 1] == np.int32(SENT)).all()


def test_row_list_and_per_clip_lengths(dev):
    """A strict, out-of-order subset of the clips; lens indexed by CLIP (not by the position in rows), len_add > 0, max_len above
    every actual length, a clip whose lens entry is 0; unlisted rows untouched.  Both with a vector stride and a scalar one."""
    rows = [5, 0, 3]
    lens = [1021, 777, 555, 0, 333, 4, 999]                    # clips 0, 3, 5 are used: 1021 + 3, 0 + 3, 4 + 3
    for stride in (1100, 1101):
        _run(dev, 7, stride, rows=rows, lens=lens, len_add=3, max_len=1090)
    _run(dev, 7, 1028, rows=rows, lens=None, len_add=1025, max_len=1028)
    _run(dev, 7, 1100, rows=None, lens=lens, len_add=1, max_len=1030)            # every clip, its own length
    a = _run(dev, 7, 8, rows=[6], len_add=5)
    assert (a[:48] == np.int32(SENT)).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_seeds(dev, seed):
    """Both halves of the 64-bit seed are key words: 2^32 + 43 and 2^63 + 1 match the reference and differ from 43."""
    a = _run(dev, 3, 1028, len_add=1025, seed=seed)
    b = _run(dev, 3, 1028, len_add=1025, seed=43)
    assert (seed == 43) == bool(np.array_equal(a, b))
    if seed != 43:
        sample = np.arange(3)[:, None] * 1028 + np.arange(1025)[None]
        assert (a[sample] != b[sample]).mean() > 0.999


@pytest.mark.parametrize("counter", COUNTERS)
def test_counters(dev, counter):
    a = _run(dev, 3, 1028, len_add=1025, counter=counter)
    b = _run(dev, 3, 1028, len_add=1025, counter=1)
    assert (counter == 1) == bool(np.array_equal(a, b))


def test_ranges(dev):
    for lo, hi in _ranges():
        body = _run(dev, 2, 4100, len_add=4099, lo=lo, hi=hi)
        v = body.reshape(2, 4100)[:, :4099].view(np.float32)
        assert (v >= np.float32(lo)).all() and (v < np.float32(hi)).all(), (lo, hi)


def test_clips_do_not_share_a_stream(dev):
    body = _run(dev, 4, 4096, len_add=4096, lo=0.0, hi=1.0).view(np.float32).reshape(4, 4096)
    for a in range(4):
        for b in range(a + 1, 4):
            assert (body[a] != body[b]).mean() > 0.999, (a, b)


def test_two_launches_give_the_same_bits(dev):
    kw = dict(rows=[2, 0], lens=[7, 0, 1020], len_add=5, max_len=1030, seed=SEEDS[1], counter=7)
    assert np.array_equal(_run(dev, 3, 1031, **kw), _run(dev, 3, 1031, **kw))


def test_argument_statuses(dev):
    """The documented statuses, before any launch: the buffer keeps every sentinel."""
    out = Out(dev, 64)
    rows, lens = dv(dev, np.array([1, 0], np.int32), np.int32), dv(dev, np.array([4, 4], np.int32), np.int32)
    ok = [out, 16, rows, 2, lens, 4, 16, 43, 1, -1.0, 1.0]

    def with_(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return a
    assert status("mx_uniform_rows", *with_(i0=None)) == ARG                     # out
    assert status("mx_uniform_rows", *with_(i3=0)) == ARG                        # n_rows <= 0
    assert status("mx_uniform_rows", *with_(i3=-1)) == ARG
    assert status("mx_uniform_rows", *with_(i6=0)) == ARG                        # max_len <= 0
    assert status("mx_uniform_rows", *with_(i6=-4)) == ARG
    assert status("mx_uniform_rows", *with_(i1=15)) == ARG                       # stride < max_len
    assert status("mx_uniform_rows", *with_(i5=-1)) == ARG                       # len_add < 0
    assert status("mx_uniform_rows", *with_(i9=1.0, i10=1.0)) == ARG             # hi <= lo
    assert status("mx_uniform_rows", *with_(i9=1.0, i10=-1.0)) == ARG
    assert status("mx_uniform_rows", *with_(i2=None, i4=None, i3=65536, i1=4, i6=4)) == UNSUPPORTED
    torch.cuda.synchronize()
    assert out.guards_intact() and out.untouched() == out.words


# ---- through the batcher ---------------------------------------------------------------------------------------------------------
N, SR, LEAD = 4410, 44100, 37
KINDS = ("flanger", "phaser", "dry")


def _batches(dev, seed):
    """The dry rows of the first two next_batch() of a fresh batcher: per batch a list of (clip, samples as int32 words)."""
    from mod_extraction_amd import data_modules
    torch.manual_seed(5)
    np.random.seed(5)
    bt = data_modules.SyntheticFxBatcher(5, N, SR, KINDS, dev, audio_seed=seed, fixed_lead=LEAD, overlap=False)
    assert bt.kinds == ["flanger", "phaser", "dry", "flanger", "phaser"]
    assert bt._src_cur.stride(0) % 4 == 2 and N % 4 == 2               # staging rows: all-scalar path; dry rows: vectors and a tail
    out = []
    for _ in range(2):
        dry, wet, _, fxp = bt.next_batch()
        torch.cuda.synchronize()
        assert [int(v) for v in fxp["lead"].cpu()] == [0, LEAD, 0, 0, LEAD]
        rows = []
        for clip, kind in enumerate(bt.kinds):
            v = bt._src_cur[clip, :N + LEAD] if kind == "phaser" else dry[clip, 0]
            rows.append((clip, kind, v.cpu().numpy().view(np.int32).copy()))
        # the phaser crops its own dry clip out of the staging row
        for clip in (1, 4):
            assert torch.equal(dry[clip, 0], bt._src_cur[clip, LEAD:LEAD + N])
        out.append(rows)
    return out, bt.peak


def test_batcher_streams(dev):
    """Batch k of a batcher with audio_seed s is the stream (s, k): non-phaser rows in the dry channel, phaser rows (lead 37) in the
    staging row, N + lead samples of it.  The two batches differ, a second batcher with the same seed reproduces them, and the
    batcher of the next DDP rank (audio_seed + 1) shares no row with them."""
    s = 43
    got, peak = _batches(dev, s)
    for k, rows in enumerate(got, 1):
        for clip, kind, v in rows:
            want = P.uniform_row(s, k, clip, v.size, -peak, peak).view(np.int32)
            assert v.size == (N + LEAD if kind == "phaser" else N)
            assert np.array_equal(v, want), (k, clip, kind)
    for (_, _, a), (_, _, b) in zip(*got):
        assert (a != b).mean() > 0.999
    again, _ = _batches(dev, s)
    for rows_a, rows_b in zip(got, again):
        for (_, _, a), (_, _, b) in zip(rows_a, rows_b):
            assert np.array_equal(a, b)
    other, _ = _batches(dev, s + 1)
    mine = [v for rows in got for _, _, v in rows]
    for rows in other:
        for _, _, v in rows:
            for w in mine:
                assert (v[:N] != w[:N]).mean() > 0.999

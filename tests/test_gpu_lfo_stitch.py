"""GPU: ``mx_lfo_stitch`` (K22, ``file_eval.stitch_lfo``) against its numpy fp64 restatement tests/helpers/lfo_stitch64.py.

Cases: n_f in {2, 5, 345} x N in {64, 22272} x hop in {N, N/2, N/4, 1000 (N = 22272 only)} x L in {N, N + 1, 3N + 17} x random
windows at amplitude 1 and 1e-4.  Gate: |got - want| <= 2^-23 max|windows| -- twice the one fp32 rounding of an fp64 value
whose own error (positions in fp64 against the helper's exact rationals, a weighted mean of bounded values) is below 1e-13.
``cover`` is equal everywhere, a second launch gives the same bits, a single window with L = N and n_t = n_f is returned bit
for bit, ``out=`` may sit at any 4-byte offset, and no output bit depends on uninitialised memory."""
import numpy as np
import pytest
import torch

from tests.helpers import lfo_stitch64 as S

pytestmark = pytest.mark.gpu

GATE = 2.0 ** -23


def hops_of(N):
    return [N, N // 2, N // 4] + ([1000] if N == 22272 else [])


def starts_of(L, N, hop):
    s = list(range(0, L - N + 1, hop))
    return s if s[-1] == L - N else s + [L - N]


@pytest.mark.parametrize("N", [64, 22272])
@pytest.mark.parametrize("n_f", [2, 5, 345])
def test_against_fp64(dev, n_f, N):
    from mod_extraction_amd.file_eval import default_track_points, stitch_lfo
    r = np.random.default_rng(1000 * n_f + N)
    worst = 0.0
    for hop in hops_of(N):
        for L in (N, N + 1, 3 * N + 17):
            starts = starts_of(L, N, hop)
            n_t = default_track_points(L, N, n_f)
            base = r.standard_normal((len(starts), n_f))
            for amp in (1.0, 1e-4):
                x = (amp * base).astype(np.float32)
                want, want_cover = S.stitch(x, starts, L, N, n_t)
                xd = torch.from_numpy(x).to(dev)
                track, cover = stitch_lfo(xd, starts, L, N)
                assert track.shape == (n_t,) and track.dtype == torch.float32 and cover.dtype == torch.int32
                assert cover.cpu().numpy().tolist() == want_cover.tolist(), (n_f, N, hop, L)
                err = float(np.abs(track.cpu().numpy().astype(np.float64) - want).max()) / float(np.abs(x).max())
                worst = max(worst, err)
                assert err <= GATE, (n_f, N, hop, L, amp, err)
                again, cover2 = stitch_lfo(xd, torch.tensor(starts, dtype=torch.int64, device=dev), L, N)
                assert torch.equal(again, track) and torch.equal(cover2, cover)
    print(f"n_f {n_f} N {N}: worst |got - want| / max|windows| = {worst:.3g} (gate {GATE:.3g})")


@pytest.mark.parametrize("N, n_f", [(64, 2), (64, 5), (64, 64), (22272, 345), (88200, 345)])
def test_one_window_is_returned_bit_for_bit(dev, N, n_f):
    from mod_extraction_amd.file_eval import stitch_lfo
    x = torch.from_numpy(np.random.default_rng(N + n_f).standard_normal((1, n_f)).astype(np.float32)).to(dev)
    track, cover = stitch_lfo(x, [0], N, N, n_t=n_f)
    assert torch.equal(track, x[0]) and bool((cover == 1).all())


def test_other_track_lengths_and_out_at_an_offset(dev):
    """n_t other than the default (2, a prime, four times the windows' rate), and ``out=`` 1, 2 and 3 floats off a 16-byte
    boundary: the same bits as a fresh output, and nothing written beside it."""
    from mod_extraction_amd.file_eval import stitch_lfo
    N, n_f, L, hop = 22272, 345, 3 * 22272 + 17, 1000
    starts = starts_of(L, N, hop)
    x = np.random.default_rng(5).standard_normal((len(starts), n_f)).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    for n_t in (2, 1031, 4140):
        want, want_cover = S.stitch(x, starts, L, N, n_t)
        track, cover = stitch_lfo(xd, starts, L, N, n_t)
        assert cover.cpu().numpy().tolist() == want_cover.tolist()
        err = float(np.abs(track.cpu().numpy().astype(np.float64) - want).max()) / float(np.abs(x).max())
        assert err <= GATE, (n_t, err)
        for off in (1, 2, 3):
            buf = torch.full((n_t + 8,), 7.0, device=dev)
            assert buf.data_ptr() % 16 == 0
            got, cover2 = stitch_lfo(xd, starts, L, N, n_t, out=buf[off:off + n_t])
            assert got.data_ptr() == buf.data_ptr() + 4 * off
            assert torch.equal(got, track) and torch.equal(cover2, cover)
            assert bool((buf[:off] == 7.0).all()) and bool((buf[off + n_t:] == 7.0).all())


def test_uninitialised_memory_changes_no_bit(dev):
    """``stitch_lfo`` takes the track and the cover from ``torch.empty``: fills of 0 / 0.5 / NaN change no bit (the probe of
    tests/test_gpu_uninit_independence.py on tests/helpers/poison_alloc.py)."""
    from mod_extraction_amd.file_eval import stitch_lfo
    from tests.test_gpu_uninit_independence import run_patterns
    N, n_f, L, hop = 22272, 345, 3 * 22272 + 17, 5568
    starts = starts_of(L, N, hop)
    xd = torch.from_numpy(np.random.default_rng(6).standard_normal((len(starts), n_f)).astype(np.float32)).to(dev)
    st = torch.tensor(starts, dtype=torch.int64, device=dev)

    def case():
        track, cover = stitch_lfo(xd, st, L, N)
        return {"track": track, "cover": cover}

    run_patterns(case, {"file_eval:stitch_lfo"})

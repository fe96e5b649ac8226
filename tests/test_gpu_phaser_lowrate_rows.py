"""GPU: the row-listed low-rate phaser kernels mx_phaser_mod_expand_rows / mx_phaser_dmod_gather_rows (csrc/phaser_lr.hip)
through fx.phaser_mod_expand(rows=) / fx.phaser_dmod_gather(rows=, out=).

For B = 5 and the row lists [0, 3, 4], [4, 1] (not ascending) and all rows: the listed rows are torch.equal to the un-listed
kernels' output (whose own accuracy tests/test_gpu_phaser_lowrate.py gates), the rows that are not listed keep the sentinel
the output was filled with, and two runs give identical bits.  An empty list launches nothing.

Shapes (N, n_mod, lead): (1, 1, 0), (4, 2, 0), (5, 2, 3), (37, 5, 6), (64, 64, 1) with per-row leads that differ within the
batch, and the step's (22272, 88) with random per-row leads."""
import pytest
import torch

pytestmark = pytest.mark.gpu
B = 5
SHAPES = [(1, 1, 0), (4, 2, 0), (5, 2, 3), (37, 5, 6), (64, 64, 1), (22272, 88, None)]
ROW_LISTS = [[0, 3, 4], [4, 1], [0, 1, 2, 3, 4]]
SENTINEL = -7.0


def leads_of(lead, N):
    if lead is None:                                                            # random per-row leads
        return torch.randint(0, 30000, (B,), generator=torch.Generator().manual_seed(N)).tolist()
    return [lead, 0, lead + 3, lead + 1, 2 * lead + 6]


@pytest.mark.parametrize("N,n_mod,lead", SHAPES)
def test_listed_rows_equal_the_unlisted_kernels(dev, N, n_mod, lead):
    from mod_extraction_amd import fx
    leads = leads_of(lead, N)
    W = N + max(leads) + 5
    ng = (W + 3) // 4
    gen = torch.Generator(device=dev).manual_seed(3 * N + n_mod)
    mod = torch.rand(B, n_mod, device=dev, generator=gen)
    buf = torch.randn(B, ng + 3, device=dev, generator=gen)
    d = buf[:, :ng]                                                             # a row stride longer than the row
    for lead_t in (torch.tensor(leads, device=dev, dtype=torch.int32), None):
        want_e = fx.phaser_mod_expand(mod, lead_t, N, W)
        want_g = fx.phaser_dmod_gather(d, lead_t, N, n_mod)
        for rows in ROW_LISTS:
            rows_t = torch.tensor(rows, device=dev, dtype=torch.int32)
            other = [b for b in range(B) if b not in rows]
            runs = []
            for _ in range(2):
                e = torch.full((B, ng + 2), SENTINEL, device=dev)               # wider than the row: the padding stays too
                g = torch.full((B, n_mod), SENTINEL, device=dev)
                assert fx.phaser_mod_expand(mod, lead_t, N, W, out=e, rows=rows_t) is e
                assert fx.phaser_dmod_gather(d, lead_t, N, n_mod, rows=rows_t, out=g) is g
                runs.append((e, g))
            (e, g), (e2, g2) = runs
            assert torch.equal(e[rows, :ng], want_e[rows]), (rows, "expand")
            assert torch.equal(g[rows], want_g[rows]), (rows, "gather")
            assert (e[:, ng:] == SENTINEL).all() and (e[other] == SENTINEL).all(), (rows, "expand wrote an unlisted row")
            assert (g[other] == SENTINEL).all(), (rows, "gather wrote an unlisted row")
            assert torch.equal(e, e2) and torch.equal(g, g2), (rows, "two runs differ")
    # an empty list launches nothing; rows=None with out= is the un-listed launch
    none = torch.empty(0, device=dev, dtype=torch.int32)
    e = torch.full((B, ng), SENTINEL, device=dev)
    g = torch.full((B, n_mod), SENTINEL, device=dev)
    fx.phaser_mod_expand(mod, None, N, W, out=e, rows=none)
    fx.phaser_dmod_gather(d, None, N, n_mod, rows=none, out=g)
    assert (e == SENTINEL).all() and (g == SENTINEL).all()
    assert torch.equal(fx.phaser_dmod_gather(d, None, N, n_mod, out=g), want_g) and torch.equal(g, want_g)


def test_forward_and_backward_lr_through_a_row_list(dev):
    """fx.phaser_forward_stash_lr / fx.phaser_backward_lr with rows=: the listed rows of the shared outputs equal the
    un-listed composition, the others keep what they held."""
    from mod_extraction_amd import fx
    N, n_mod, sr = 4096, 41, 44100.0
    gen = torch.Generator(device=dev).manual_seed(5)
    x = 0.5 * (2.0 * torch.rand(B, N, device=dev, generator=gen) - 1.0)
    mod = torch.rand(B, n_mod, device=dev, generator=gen)
    dy = torch.randn(B, N, device=dev, generator=gen)
    params = {"depth": torch.tensor([0.2, 1.0, 1.0, 0.5, 0.8], device=dev),
              "centre_frequency_hz": torch.tensor([70.0, 440.0, 1300.0, 5000.0, 18000.0], device=dev),
              "feedback": torch.tensor([-0.7, 0.0, 0.25, 0.7, 0.5], device=dev),
              "mix": torch.tensor([0.2, 1.0, 0.7, 1.0, 0.5], device=dev)}
    y0, st0, _ = fx.phaser_forward_stash_lr(x, params, None, sr, N, mod)
    _, dmod0, _ = fx.phaser_backward_lr(dy, x, st0, params, None, sr, N, n_mod, need_dx=False, params_wanted=())
    for rows in ([4, 1], [0, 3, 4]):
        rows_t = torch.tensor(rows, device=dev, dtype=torch.int32)
        other = [b for b in range(B) if b not in rows]
        y = torch.full((B, N), SENTINEL, device=dev)
        dmod = torch.full((B, n_mod), SENTINEL, device=dev)
        y1, st, _ = fx.phaser_forward_stash_lr(x, params, None, sr, N, mod, rows=rows_t, out=y)
        _, d1, _ = fx.phaser_backward_lr(dy, x, st, params, None, sr, N, n_mod, need_dx=False, params_wanted=(), rows=rows_t,
                                         dmod=dmod)
        assert y1 is y and d1 is dmod
        assert torch.equal(y[rows], y0[rows]) and torch.equal(dmod[rows], dmod0[rows])
        assert (y[other] == SENTINEL).all() and (dmod[other] == SENTINEL).all()
    none = torch.empty(0, device=dev, dtype=torch.int32)
    y = torch.full((B, N), SENTINEL, device=dev)
    dmod = torch.full((B, n_mod), SENTINEL, device=dev)
    _, st, _ = fx.phaser_forward_stash_lr(x, params, None, sr, N, mod, rows=none, out=y)
    fx.phaser_backward_lr(dy, x, st, params, None, sr, N, n_mod, need_dx=False, params_wanted=(), rows=none, dmod=dmod)
    assert (y == SENTINEL).all() and (dmod == SENTINEL).all()

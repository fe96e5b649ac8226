"""GPU: the tremolo kernels (csrc/tremolo.hip) behind fx.tremolo_forward / tremolo_backward / TremoloModule.

* forward, bit for bit: the reference's own vectors (tests/golden/rand_lfo_tremolo.npz, from the real fx.py:13-22), and a
  low-rate LFO against the two-step composition on the device -- util.linear_interpolate_last_dim, then the torch
  expression of fx.py:22 -- over N in {1, 5, 63, 64, 257, 4099} x n_mod in {1, 2, N - 1, N, N // 100}, mix in
  {0, 1, 0.37} as a python float and as a (B,) tensor;
* views and the rows list: channel 1 of a (B, 2, 4099) tensor (odd N: the rows are not 16-byte aligned, the scalar path)
  and rows = [2, 0] into a sentinel-filled output;
* the adjoint against tests/helpers/tremolo_adjoint64.py with the project's gates for these quantities
  (tests/test_gpu_flanger_grad.py, test_gpu_flanger_lowrate_grad.py): dx 2e-6, dmod 3e-6, dmix 1e-5, norm-wise;
* output selection and run-to-run bit-identity; TremoloModule under torch.autograd with two channels."""
import os

import numpy as np
import pytest
import torch

from tests.helpers.tremolo_adjoint64 import tremolo_adjoint64
from tests.test_gpu_flanger_grad import normwise

pytestmark = pytest.mark.gpu
B = 3
MIXES = (0.0, 1.0, 0.37)


def n_mods(N):
    out = []
    for m in (1, 2, N - 1, N) + ((N // 100,) if N // 100 >= 2 else ()):
        m = min(max(m, 1), N)
        if m not in out:
            out.append(m)
    return out


GRID = [(N, m) for N in (1, 5, 63, 64, 257, 4099) for m in n_mods(N)]


def inputs(dev, N, n_mod, seed=0):
    g = torch.Generator().manual_seed(1000 * N + n_mod + seed)
    x = (torch.rand(B, N, generator=g) * 2 - 1).to(dev)
    mod = torch.rand(B, n_mod, generator=g).to(dev)
    dy = torch.randn(B, N, generator=g).to(dev)
    return x, mod, dy


def two_step(x, mod, mix):
    """fx.py:22 as separate torch ops on the resampled LFO: the route apply_tremolo took before the kernel."""
    from mod_extraction_amd.util import linear_interpolate_last_dim
    m = linear_interpolate_last_dim(mod, x.size(-1), align_corners=True)
    if isinstance(mix, torch.Tensor):
        mix = mix[:, None]
    return ((1.0 - mix) * x) + (mix * m * x)


def test_forward_reference_vectors_bit_exact(golden_dir, dev):
    from mod_extraction_amd import fx
    g = np.load(os.path.join(golden_dir, "rand_lfo_tremolo.npz"))
    x, mod = torch.from_numpy(g["trem_x"]).to(dev), torch.from_numpy(g["trem_mod"]).to(dev)
    bs, n_ch, n = x.shape
    assert bs == B
    xr, mr = x.reshape(bs * n_ch, n), mod.repeat_interleave(n_ch, 0).contiguous()
    for mix, key in ((0.7, "trem_y_07"), (1.0, "trem_y_10"), (0.0, "trem_y_00")):
        consts = fx.derive_tremolo_constants(bs * n_ch, dev, mix)
        y = fx.tremolo_forward(xr, mr, consts).view(bs, n_ch, n)
        assert torch.equal(y.cpu(), torch.from_numpy(g[key])), key
        assert torch.equal(fx.apply_tremolo(x, mod, mix).cpu(), torch.from_numpy(g[key])), key
        assert torch.equal(fx.TremoloModule()(x, mod, mix).cpu(), torch.from_numpy(g[key])), key


@pytest.mark.parametrize("N,n_mod", GRID)
def test_low_rate_equals_two_step_composition(dev, N, n_mod):
    from mod_extraction_amd import fx
    x, mod, _ = inputs(dev, N, n_mod)
    per_clip = torch.tensor(MIXES, device=dev)
    for mix in MIXES + tuple(torch.full((B,), v, device=dev) for v in MIXES) + (per_clip,):
        y = fx.tremolo_forward(x, mod, fx.derive_tremolo_constants(B, dev, mix))
        assert torch.equal(y, two_step(x, mod, mix)), mix


@pytest.mark.parametrize("n_mod", [40, 4099])
def test_views_and_rows(dev, n_mod):
    from mod_extraction_amd import fx
    N = 4099
    x, mod, dy = inputs(dev, N, n_mod, seed=1)
    consts = fx.derive_tremolo_constants(B, dev, torch.tensor([0.37, 1.0, 0.6], device=dev))
    dense = fx.tremolo_forward(x, mod, consts)
    buf = torch.zeros(B, 2, N, device=dev)
    buf[:, 1, :] = x
    out = torch.full((B, 2, N), -7.0, device=dev)
    xv, ov = buf[:, 1, :], out[:, 1, :]
    assert xv.data_ptr() % 16 != 0 and xv.stride(0) == 2 * N           # channel 1, odd N: misaligned rows
    assert fx.tremolo_forward(xv, mod, consts, out=ov).data_ptr() == ov.data_ptr()
    assert torch.equal(ov, dense) and bool((out[:, 0, :] == -7.0).all())
    rows = torch.tensor([2, 0], dtype=torch.int32, device=dev)
    for src in (x, xv):
        out = torch.full((B, 2, N), -7.0, device=dev)
        fx.tremolo_forward(src, mod, consts, rows=rows, out=out[:, 1, :])
        assert torch.equal(out[[2, 0], 1, :], dense[[2, 0]])
        assert bool((out[1] == -7.0).all()) and bool((out[:, 0, :] == -7.0).all())
    # the adjoint on the same views: the per-sample and per-point outputs do not depend on the load width
    gbuf = torch.zeros(B, 2, N, device=dev)
    gbuf[:, 1, :] = dy
    a = fx.tremolo_backward(dy, x, mod, consts)
    b = fx.tremolo_backward(gbuf[:, 1, :], xv, mod, consts)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert float(((a[2] - b[2]).abs() / a[2].abs()).max()) <= 1e-12     # the fp64 partial sums are grouped by 4 / by 1
    c = fx.tremolo_backward(dy, x, mod, consts, rows=rows)
    assert torch.equal(c[0][[2, 0]], a[0][[2, 0]]) and torch.equal(c[1][[2, 0]], a[1][[2, 0]])
    assert torch.equal(c[2][[2, 0]], a[2][[2, 0]])
    assert float(c[0][1].abs().max()) == 0.0 and float(c[1][1].abs().max()) == 0.0 and float(c[2][1]) == 0.0


@pytest.mark.parametrize("N,n_mod", [c for c in GRID if c[0] >= 5])
def test_adjoint_against_fp64(dev, N, n_mod):
    from mod_extraction_amd import fx
    x, mod, dy = inputs(dev, N, n_mod, seed=2)
    consts = fx.derive_tremolo_constants(B, dev, torch.tensor([0.37, 1.0, 0.05], device=dev))
    dx, dmod, dmix = fx.tremolo_backward(dy, x, mod, consts)
    assert dx.shape == (B, N) and dmod.shape == (B, n_mod) and dmix.shape == (B,) and dmix.dtype == torch.float64
    ref = tremolo_adjoint64(x.cpu().numpy(), mod.cpu().numpy(), consts["mix"].cpu().numpy(), dy.cpu().numpy(),
                            omm=consts["one_minus_mix"].cpu().numpy())
    e_dx = normwise(dx.cpu().numpy(), ref["dx"], slice(None))
    e_dmod = normwise(dmod.cpu().numpy(), ref["dmod"], slice(None))
    e_dmix = normwise(dmix.cpu().numpy(), ref["dmix"], slice(None))
    print(f"N {N} n_mod {n_mod}: dx {e_dx:.3g} dmod {e_dmod:.3g} dmix {e_dmix:.3g}")
    assert e_dx <= 2e-6
    assert e_dmod <= 3e-6
    assert e_dmix <= 1e-5


@pytest.mark.parametrize("n_mod", [40, 4099])
def test_output_selection_and_determinism(dev, n_mod):
    from mod_extraction_amd import fx
    N = 4099
    x, mod, dy = inputs(dev, N, n_mod, seed=3)
    consts = fx.derive_tremolo_constants(B, dev, 0.8)
    dx, dmod, dmix = fx.tremolo_backward(dy, x, mod, consts)
    none_dx, dmod_only, none_dmix = fx.tremolo_backward(dy, x, mod, consts, need_dx=False, need_dmix=False)
    assert none_dx is None and none_dmix is None and torch.equal(dmod_only, dmod)
    _, dmod2, _ = fx.tremolo_backward(dy, x, mod, consts, need_dx=False)
    assert torch.equal(dmod2, dmod)
    dx3, none_dmod, dmix3 = fx.tremolo_backward(dy, x, mod, consts, need_dmod=False)
    assert none_dmod is None and torch.equal(dx3, dx) and torch.equal(dmix3, dmix)
    again = fx.tremolo_backward(dy, x, mod, consts)
    assert torch.equal(again[0], dx) and torch.equal(again[1], dmod) and torch.equal(again[2], dmix)


def test_module_autograd_two_channels(dev):
    from mod_extraction_amd import fx
    n_ch, N, n_mod = 2, 257, 7
    g = torch.Generator().manual_seed(9)
    x = (torch.rand(B, n_ch, N, generator=g) * 2 - 1).to(dev).requires_grad_(True)
    mod = torch.rand(B, n_mod, generator=g).to(dev).requires_grad_(True)
    mix = torch.tensor([0.37, 1.0, 0.05], device=dev, requires_grad=True)
    w = torch.randn(B, n_ch, N, generator=g).to(dev)
    module = fx.TremoloModule()
    y = module.apply_effect(x, mod, mix)
    assert y.grad_fn is not None and y.shape == x.shape
    assert torch.equal(y.detach(), module(x, mod, mix)) and module(x, mod, mix).grad_fn is None
    assert module.apply_effect(x.detach(), mod.detach(), 0.5).grad_fn is None
    y.sum().backward()                                                  # an expanded dy
    assert x.grad.shape == x.shape and mod.grad.shape == mod.shape and mix.grad.shape == mix.shape
    ones = x.grad.clone()
    x.grad = mod.grad = mix.grad = None
    (module.apply_effect(x, mod, mix) * w).sum().backward()
    assert not torch.equal(x.grad, ones)
    c = fx.derive_tremolo_constants(B, dev, mix.detach())
    xs, ws = x.detach().cpu().numpy(), w.cpu().numpy()
    refs = [tremolo_adjoint64(xs[:, c_], mod.detach().cpu().numpy(), c["mix"].cpu().numpy(), ws[:, c_],
                              omm=c["one_minus_mix"].cpu().numpy()) for c_ in range(n_ch)]
    e_dx = normwise(x.grad.cpu().numpy(), np.stack([r["dx"] for r in refs], 1), slice(None))
    e_dmod = normwise(mod.grad.cpu().numpy(), sum(r["dmod"] for r in refs), slice(None))
    e_dmix = normwise(mix.grad.cpu().numpy(), sum(r["dmix"] for r in refs), slice(None))
    print(f"module, 2 channels: dx {e_dx:.3g} dmod {e_dmod:.3g} dmix {e_dmix:.3g}")
    assert e_dx <= 2e-6
    assert e_dmod <= 3e-6
    assert e_dmix <= 1e-5
    # a channel axis on mod_sig: (B, 1, n_mod) is shared, (B, n_ch, n_mod) is per channel
    m3 = torch.rand(B, n_ch, n_mod, generator=g).to(dev)
    y3 = module(x.detach(), m3, 0.37)
    for c_ in range(n_ch):
        assert torch.equal(y3[:, c_:c_ + 1], module(x.detach()[:, c_:c_ + 1], m3[:, c_:c_ + 1], 0.37))

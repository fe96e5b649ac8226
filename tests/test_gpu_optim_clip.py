"""GPU: gradient clipping on the device (csrc/optim_clip.hip) -- mx_grad_sumsq against fp64, mx_adamw_step_clip bit for bit
against mx_adamw_step with the host-restated scale, and FlatAdamW with a clip against torch's clip_grad_norm_ /
clip_grad_value_ + AdamW on the CPU."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK, CAP = 4096, 1024                     # optim.SUMSQ_CHUNK / SUMSQ_MAX_PARTIALS (asserted below)
HP = dict(lr=1e-3, beta1=0.8, beta2=0.99, eps=1e-8, wd=0.01)
SENTINEL = -7.0


def _sumsq(g, part, stat):
    from mod_extraction_amd import _hip
    _hip.call("mx_grad_sumsq", _hip.ptr(g), g.numel(), _hip.ptr(part), _hip.ptr(stat), _hip.stream())


def _adamw(p, g, m, v, step, grad_scale):
    from mod_extraction_amd import _hip
    _hip.call("mx_adamw_step", _hip.ptr(p), _hip.ptr(g), _hip.ptr(m), _hip.ptr(v), p.numel(), step, HP["lr"], HP["beta1"],
              HP["beta2"], HP["eps"], HP["wd"], grad_scale, _hip.stream())


def _adamw_clip(p, g, m, v, step, grad_scale, mode, clip_val, stat):
    from mod_extraction_amd import _hip
    _hip.call("mx_adamw_step_clip", _hip.ptr(p), _hip.ptr(g), _hip.ptr(m), _hip.ptr(v), p.numel(), step, HP["lr"], HP["beta1"],
              HP["beta2"], HP["eps"], HP["wd"], grad_scale, mode, clip_val, _hip.ptr(stat), _hip.stream())


def _state(n, dev, seed):
    """A mid-training optimizer state (non-zero moments) and a gradient."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen)
    m = torch.randn(n, generator=gen) * 0.1
    v = torch.rand(n, generator=gen) * 0.01
    return [t.to(dev) for t in (p, g, m, v)]


def _host_scale(sumsq: float, grad_scale: float, clip_val: float) -> float:
    """The scale of mx_adamw_step_clip's norm mode restated on the host (include/modex_hip.h): Python floats are fp64,
    math.sqrt and / are correctly rounded like the device's, the result is rounded once to fp32."""
    norm = math.sqrt(sumsq) * grad_scale
    coef = min(1.0, clip_val / (norm + 1e-6))
    return float(np.float32(grad_scale * coef))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 17, CAP * CHUNK + 5])
def test_grad_sumsq_vs_fp64(dev, n):
    from mod_extraction_amd import optim
    assert (optim.SUMSQ_CHUNK, optim.SUMSQ_MAX_PARTIALS) == (CHUNK, CAP)
    G = optim.sumsq_partials(n)
    assert G == min(-(-n // CHUNK), CAP)
    rng = np.random.default_rng(n)
    g_np = (rng.standard_normal(n) * 10.0 ** rng.uniform(-12.0, 3.0, n)).astype(np.float32)
    g = torch.from_numpy(g_np).to(dev)
    keep = g.clone()
    part = torch.full((G + 8,), SENTINEL, device=dev, dtype=torch.float64)
    stat = torch.full((8,), SENTINEL, device=dev, dtype=torch.float64)
    _sumsq(g, part, stat)
    part1, stat1 = part.clone(), stat.clone()
    _sumsq(g, part, stat)
    assert torch.equal(part, part1) and torch.equal(stat, stat1)                  # no atomics: the same bits again
    assert torch.equal(g, keep)                                                   # the gradient is only read
    assert bool((part[G:] == SENTINEL).all()) and bool((stat[1:] == SENTINEL).all())
    ref = float(np.sum(g_np.astype(np.float64) ** 2, dtype=np.float64))
    got = float(stat[0])
    rel = abs(got - ref) / ref
    tol = n * 2.0 ** -53            # exact squares, positive terms: the bound of ANY summation order of n terms
    print(f"mx_grad_sumsq n={n} G={G}: relative error {rel:.3g} (bound {tol:.3g})")
    assert rel <= tol


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("n", [1, 257, 2048 * 256 + 3])
def test_norm_clip_active_equals_the_plain_step_at_the_restated_scale(dev, n, grad_scale):
    from mod_extraction_amd import optim
    p, g, m, v = _state(n, dev, seed=n)
    part = torch.zeros(optim.sumsq_partials(n), device=dev, dtype=torch.float64)
    stat = torch.zeros(2, device=dev, dtype=torch.float64)
    _sumsq(g, part, stat)
    sumsq = float(stat[0])
    clip_val = float(np.float32(0.37 * math.sqrt(sumsq) * grad_scale))           # well below the norm: the clip binds
    s = _host_scale(sumsq, grad_scale, clip_val)
    assert 0.0 < s < 0.5 * grad_scale
    ref = [t.clone() for t in (p, g, m, v)]
    _adamw(*ref, 3, s)
    keep = g.clone()
    _adamw_clip(p, g, m, v, 3, grad_scale, 1, clip_val, stat)
    assert float(stat[1]) == s and float(stat[0]) == sumsq
    assert torch.equal(p, ref[0]) and torch.equal(m, ref[2]) and torch.equal(v, ref[3])
    assert torch.equal(g, keep)                                                   # grad stays un-clipped


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("n", [1, 257, 2048 * 256 + 3])
def test_norm_clip_that_does_not_bind_is_the_plain_step(dev, n, grad_scale):
    from mod_extraction_amd import optim
    p, g, m, v = _state(n, dev, seed=n + 1)
    part = torch.zeros(optim.sumsq_partials(n), device=dev, dtype=torch.float64)
    stat = torch.zeros(2, device=dev, dtype=torch.float64)
    ref = [t.clone() for t in (p, g, m, v)]
    _adamw(*ref, 1, grad_scale)
    _sumsq(g, part, stat)
    _adamw_clip(p, g, m, v, 1, grad_scale, 1, 1e30, stat)
    assert float(stat[1]) == grad_scale
    assert torch.equal(p, ref[0]) and torch.equal(m, ref[2]) and torch.equal(v, ref[3])


@pytest.mark.parametrize("n", [1, 257, 2048 * 256 + 3])
def test_value_clip_equals_the_plain_step_on_the_clamped_gradient(dev, n):
    c, grad_scale = float(np.float32(0.3)), 0.5
    p, g, m, v = _state(n, dev, seed=n + 2)
    stat = torch.full((2,), SENTINEL, device=dev, dtype=torch.float64)
    clamped = torch.clamp(g * grad_scale, -c, c)
    if n > 1:
        assert bool((clamped == c).any()) and bool((clamped == -c).any()) and bool((clamped.abs() < c).any())
    ref = [p.clone(), clamped, m.clone(), v.clone()]
    _adamw(*ref, 2, 1.0)
    keep = g.clone()
    _adamw_clip(p, g, m, v, 2, grad_scale, 2, c, stat)
    assert torch.equal(p, ref[0]) and torch.equal(m, ref[2]) and torch.equal(v, ref[3]) and torch.equal(g, keep)
    assert float(stat[0]) == SENTINEL and float(stat[1]) == grad_scale           # stat[0] is not touched in value mode


def test_value_clip_propagates_a_nan_like_torch_clamp(dev):
    n, bad = 257, 100
    p, g, m, v = _state(n, dev, seed=9)
    g[bad] = float("nan")
    stat = torch.zeros(2, device=dev, dtype=torch.float64)
    _adamw_clip(p, g, m, v, 1, 1.0, 2, 0.3, stat)
    ok = torch.ones(n, dtype=torch.bool, device=dev)
    ok[bad] = False
    assert bool(torch.isnan(p[bad])) and bool(torch.isnan(m[bad])) and bool(torch.isnan(v[bad]))
    assert bool(torch.isfinite(p[ok]).all()) and bool(torch.isfinite(m[ok]).all()) and bool(torch.isfinite(v[ok]).all())


@pytest.mark.parametrize("algorithm,clip_val", [("norm", 0.5), ("value", 0.01)])
def test_flat_adamw_with_a_clip_vs_torch(dev, algorithm, clip_val):
    """The set-up of test_adamw_kernel_vs_torch (three tensors, gradient scales 10^-step, lr 1e-4, the DDP 1/world path) with
    torch's own clip in front of torch.optim.AdamW.  Norm mode at 0.5: steps 0-2 are clipped, steps 3-4 are not."""
    from mod_extraction_amd import optim
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(64, 2, 5, 13)), torch.nn.Parameter(torch.randn(64)),
          torch.nn.Parameter(torch.randn(1, 64, 1))]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    mine = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in ps]
    o_ref = torch.optim.AdamW(ref, lr=1e-4, betas=(0.8, 0.99))
    o_mine = optim.FlatAdamW(mine, lr=1e-4, betas=(0.8, 0.99), clip_val=clip_val, clip_algorithm=algorithm)
    for step in range(5):
        grads = [torch.randn_like(p) * (10.0 ** -step) for p in ps]
        for p, g in zip(ref, grads):
            p.grad = g.clone()
        o_mine.zero_grad()
        for p, g in zip(mine, grads):
            p.grad.copy_(g.to(dev) * 2.0)          # grad_scale 0.5 undoes this (the DDP 1/world path)
        if algorithm == "norm":
            norm_ref = float(torch.nn.utils.clip_grad_norm_(ref, clip_val))
        else:
            torch.nn.utils.clip_grad_value_(ref, clip_val)
        o_ref.step()
        o_mine.step(grad_scale=0.5)
        err = max(float((p.detach().cpu() - q.detach()).abs().max()) for p, q in zip(mine, ref))
        print(f"FlatAdamW clip {algorithm} step {step}: max abs parameter error {err:.3g}")
        assert err < 3e-7, step
        for p, g in zip(mine, grads):              # the flat gradient itself stays un-clipped
            assert torch.equal(p.grad.cpu(), g * 2.0)
        scale = float(o_mine.last_clip_scale)
        if algorithm == "norm":
            assert o_mine.last_grad_norm.is_cuda and o_mine.last_clip_scale.is_cuda
            rel = abs(float(o_mine.last_grad_norm) - norm_ref) / norm_ref
            print(f"FlatAdamW clip norm step {step}: norm {float(o_mine.last_grad_norm):.6g}, relative to torch's {rel:.3g}")
            assert rel < 1e-6, step
            assert (scale < 0.5) if step <= 2 else (scale == 0.5), (step, scale)
        else:
            assert o_mine.last_grad_norm is None and scale == 0.5
    assert o_mine.step_count == 5


def _spy(monkeypatch):
    from mod_extraction_amd import _hip
    names, real = [], _hip.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(_hip, "call", call)
    return names


def _rows_optimizers(dev, **kw):
    from mod_extraction_amd import optim
    torch.manual_seed(3)
    w = torch.randn(17473)
    part = (torch.randn(7, 17473) * 3.0).to(dev)                                  # one gradient row per clip (TBPTT shape)
    return [optim.FlatAdamW([torch.nn.Parameter(w.clone().to(dev))], lr=1e-3, betas=(0.8, 0.99), **kw) for _ in range(2)], part


def _same(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("flat_param", "flat_grad", "exp_avg", "exp_avg_sq"))


@pytest.mark.parametrize("algorithm", ["norm", "value"])
def test_step_from_rows_with_a_clip_is_reduce_rows_then_step(dev, monkeypatch, algorithm):
    from mod_extraction_amd import _hip
    (a, b), part = _rows_optimizers(dev, clip_val=1.0, clip_algorithm=algorithm)
    names = _spy(monkeypatch)
    for _ in range(2):
        del names[:]
        a.step_from_rows(part, grad_scale=0.5)
        assert names == ["mx_reduce_rows"] + (["mx_grad_sumsq"] if algorithm == "norm" else []) + ["mx_adamw_step_clip"]
        _hip.call("mx_reduce_rows", _hip.ptr(part), 7, 17473, 0, _hip.ptr(b.flat_grad), _hip.stream())
        b.step(grad_scale=0.5)
    assert _same(a, b) and a.step_count == b.step_count == 2
    assert torch.equal(a.last_clip_scale, b.last_clip_scale) and float(a.last_clip_scale) <= 0.5
    if algorithm == "norm":
        assert float(a.last_clip_scale) < 0.5 and torch.equal(a.last_grad_norm, b.last_grad_norm)


def test_step_from_rows_and_step_without_a_clip_make_the_parents_launches(dev, monkeypatch):
    from mod_extraction_amd import _hip
    (a, b), part = _rows_optimizers(dev)
    names = _spy(monkeypatch)
    a.step_from_rows(part, grad_scale=0.5)
    assert names == ["mx_reduce_rows_adamw_step"]
    b.step_count += 1
    _hip.call("mx_reduce_rows_adamw_step", _hip.ptr(part), 7, _hip.ptr(b.flat_param), _hip.ptr(b.flat_grad), _hip.ptr(b.exp_avg),
              _hip.ptr(b.exp_avg_sq), 17473, 1, 1e-3, 0.8, 0.99, 1e-8, 0.01, 0.5, _hip.stream())
    assert _same(a, b)
    del names[:]
    a.set_gradient_clip(0.0, "norm")                                              # <= 0: still off
    a.step(grad_scale=0.5)
    assert names == ["mx_adamw_step"] and a.last_clip_scale is None

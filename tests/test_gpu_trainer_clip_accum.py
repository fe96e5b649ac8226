"""GPU: gradient accumulation and clipping through `trainer.Trainer` on the real kernels -- the module, clips and seeds of the
two-rank equivalence test (tests/helpers/clip_accum_worker.py), one optimizer step each."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plain(dev):
    """ONE plain optimizer step on the joined batch of 4 clips (the reference of every test here), and its twin with a clip
    that cannot bind, which records the norm of the gradient."""
    from tests.helpers import clip_accum_worker as w
    module, opt, batch = w.lfo_setup(dev)
    w.fit_once(module, opt, [batch(slice(0, 4))])
    assert opt.step_count == 1 and opt.last_clip_scale is None
    module2, twin, batch2 = w.lfo_setup(dev)
    w.fit_once(module2, twin, [batch2(slice(0, 4))], gradient_clip_val=1e30)
    assert twin.clip_val == 1e30 and float(twin.last_clip_scale) == 1.0
    assert torch.equal(twin.flat_param, opt.flat_param) and torch.equal(twin.flat_grad, opt.flat_grad)
    norm = float(twin.last_grad_norm)
    assert math.isfinite(norm) and norm > 0.0
    return {"param": opt.flat_param.cpu(), "grad": opt.flat_grad.cpu(), "norm": norm}


def _assert_same_step(a_param, a_grad, b_param, b_grad, what):
    """The gates of test_two_rank_step_equals_the_single_process_step_on_the_joined_batch (mode "lfo")."""
    g_err = float((a_grad - b_grad).abs().max()) / float(a_grad.abs().max())
    d = (a_param - b_param).abs()
    med, q = float(d.median()), float(torch.quantile(d[:: max(1, d.numel() // 100000)], 0.999))
    print(f"{what}: gradient error / max {g_err:.3g}, parameter difference median {med:.3g}, 0.999-quantile {q:.3g}")
    assert g_err < 1e-5
    assert med < 1e-6
    assert q < 2e-5


def test_two_accumulated_micro_batches_equal_one_step_on_the_joined_batch(dev, plain):
    from tests.helpers import clip_accum_worker as w
    module, opt, batch = w.lfo_setup(dev)
    w.fit_once(module, opt, [batch(slice(0, 2)), batch(slice(2, 4))], accumulate_grad_batches=2)
    assert opt.step_count == 1
    # the buffer holds the SUM of the two micro-batch gradients; the step applied it at grad_scale 1/2
    _assert_same_step(plain["param"], plain["grad"], opt.flat_param.cpu(), opt.flat_grad.cpu() / 2, "accumulate 2 x 2 clips")


def test_clip_through_the_trainer_is_the_plain_kernel_at_the_restated_scale(dev, plain):
    from mod_extraction_amd import _hip
    from tests.helpers import clip_accum_worker as w
    clip_val = float(np.float32(0.5 * plain["norm"]))
    module, opt, batch = w.lfo_setup(dev)
    before = [t.clone() for t in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq)]
    w.fit_once(module, opt, [batch(slice(0, 4))], gradient_clip_val=clip_val)
    assert opt.step_count == 1 and (opt.clip_val, opt.clip_algorithm) == (clip_val, "norm")
    sumsq = float(opt._clip_stat[0])
    norm = math.sqrt(sumsq) * 1.0
    s = float(np.float32(1.0 * min(1.0, clip_val / (norm + 1e-6))))             # include/modex_hip.h, mode 1, grad_scale 1
    assert float(opt.last_clip_scale) == s and 0.49 < s < 0.51
    assert abs(float(opt.last_grad_norm) - norm) <= 1e-15 * norm
    assert abs(norm - plain["norm"]) <= 1e-12 * norm                               # same step as the twin
    p, m, v = before
    _hip.call("mx_adamw_step", _hip.ptr(p), _hip.ptr(opt.flat_grad), _hip.ptr(m), _hip.ptr(v), p.numel(), 1, opt.lr,
              opt.betas[0], opt.betas[1], opt.eps, opt.weight_decay, s, _hip.stream())
    assert torch.equal(p, opt.flat_param) and torch.equal(m, opt.exp_avg) and torch.equal(v, opt.exp_avg_sq)
    assert not torch.equal(opt.flat_param.cpu(), plain["param"])                   # the clip changed the step
    assert torch.equal(opt.flat_grad.cpu(), plain["grad"])                         # and left the gradient un-clipped


def test_two_ranks_with_a_clip_equal_the_single_process_and_agree_bit_for_bit(dev, plain, tmp_path):
    from tests.helpers import clip_accum_worker as w
    from tests.helpers.torchrun import run_torchrun
    clip_val = float(np.float32(0.5 * plain["norm"]))
    module, opt, batch = w.lfo_setup(dev)                                          # first leg: one process, joined batch
    w.fit_once(module, opt, [batch(slice(0, 4))], gradient_clip_val=clip_val)
    assert opt.step_count == 1 and float(opt.last_clip_scale) < 0.51
    out = str(tmp_path / "two.pt")
    env = dict(os.environ, MODEX_SHARE_GPU="1", MODEX_DIST_BACKEND="gloo")
    res = run_torchrun(2, [os.path.join(ROOT, "tests", "helpers", "clip_accum_worker.py"), out, "4", repr(clip_val)], env=env,
                       timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    r0, r1 = torch.load(out + ".rank0"), torch.load(out + ".rank1")
    assert r0["world"] == r1["world"] == 2 and r0["steps"] == r1["steps"] == 1
    # the norm is taken of the all-reduced buffer: identical bits on both ranks, so they form the same scale without a collective
    assert torch.equal(r0["norm"], r1["norm"]) and torch.equal(r0["scale"], r1["scale"])
    assert torch.equal(r0["param"], r1["param"])
    assert 0.24 < float(r0["scale"]) < 0.26                                        # 1/world times a coefficient of ~1/2
    _assert_same_step(opt.flat_param.cpu(), opt.flat_grad.cpu(), r0["param"], r0["grad"], "two ranks with a clip")


def test_manual_optimization_module_refuses_trainer_keys_and_clips_through_its_optimizer(dev, monkeypatch):
    from mod_extraction_amd import _hip, trainer
    from tests.helpers import clip_accum_worker as w
    module, opt, batch = w.tbptt_setup(dev, clip_val=1e-3)
    assert module.automatic_optimization is False
    for kw in (dict(gradient_clip_val=1.0), dict(accumulate_grad_batches=2)):
        with pytest.raises(ValueError, match="clip_val"):
            trainer.Trainer(max_epochs=1, log_fn=None, **kw).fit(module, w.ListData([batch]), opt)
    assert opt.step_count == 0 and opt.clip_val == 1e-3
    names, real = [], _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    module.training_step(batch, 0, optimizer=opt, world_size=1)
    torch.cuda.synchronize()
    assert opt.step_count == 4                                                     # 4 chunks of 1024 samples: 4 inner steps
    assert names.count("mx_adamw_step_clip") == 4 and names.count("mx_grad_sumsq") == 4
    assert "mx_adamw_step" not in names and "mx_reduce_rows_adamw_step" not in names
    scale = float(opt.last_clip_scale)
    assert 0.0 < scale <= 1.0 and bool(torch.isfinite(opt.flat_param).all())

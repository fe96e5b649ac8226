"""GPU: K3 phaser, K9 corner bookkeeping, K12 AdamW, the on-device batch synthesis and one full
LFOExtraction train step against the CPU oracle."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import fx as ofx, lightning as ol, models as om, modulations as omod

pytestmark = pytest.mark.gpu


def test_phaser_vs_oracle(dev):
    """K3 against oracle_ref.c:orc_phaser (pedalboard/JUCE restatement; parity with pedalboard itself is
    unpinned).  Tolerance 1e-5 absolute on [-1,1] audio: device sin/pow/tan differ in the last ulp."""
    from mod_extraction_amd import fx as afx
    torch.manual_seed(2)
    B, N = 5, 30000
    lead = torch.tensor([0, 1000, 3, 14701, 257], dtype=torch.int32)
    src = torch.rand(B, N + 14701) * 1.6 - 0.8
    p = {"rate_hz": torch.tensor([0.5, 3.0, 1.3, 2.2, 0.9]), "depth": torch.tensor([1.0, 0.2, 0.6, 0.9, 0.5]),
         "centre_frequency_hz": torch.tensor([70.0, 18000.0, 440.0, 1300.0, 5000.0]),
         "feedback": torch.tensor([0.0, 0.7, 0.25, 0.5, 0.69]), "mix": torch.tensor([1.0, 0.2, 0.5, 0.8, 1.0])}
    y = torch.empty(B, N, device=dev)
    y_exact = torch.empty(B, N, device=dev)
    dry = torch.empty(B, N, device=dev)
    pd = {k: v.to(dev) for k, v in p.items()}
    afx.phaser_forward(src.to(dev), pd, lead.to(dev), 44100.0, N, out=y, dry_out=dry)                  # FMA form
    afx.phaser_forward(src.to(dev), pd, lead.to(dev), 44100.0, N, out=y_exact, exact_order=True)       # JUCE order
    assert float((y - y_exact).abs().max()) < 5e-6
    for b in range(B):
        L = int(lead[b])
        ref = ofx.phaser_np(src[b:b + 1, :L + N].numpy(), [float(p["rate_hz"][b])], [float(p["depth"][b])],
                            [float(p["centre_frequency_hz"][b])], [float(p["feedback"][b])], [float(p["mix"][b])], 44100.0)
        assert np.array_equal(dry[b].cpu().numpy(), src[b, L:L + N].numpy())
        for name, out in (("fma", y), ("exact", y_exact)):
            err = np.abs(out[b].cpu().numpy() - ref[0, L:]).max()
            assert err < 1e-5, (name, b, err)


@pytest.mark.parametrize("k", [0, 4, 8])
def test_corner_bookkeeping_bit_exact(golden_dir, dev, k):
    """K9 vs the golden vectors captured from the reference's modulations.py: ==, not allclose."""
    from mod_extraction_amd import modulations as amod
    g = np.load(os.path.join(golden_dir, "corners.npz"))
    m = torch.from_numpy(g["mod_sig"]).to(dev)
    ms = amod.smoothen(m, k)
    assert np.array_equal(ms.cpu().numpy(), g[f"smooth_{k}"])
    top, bot = amod.find_corners(ms)
    assert np.array_equal(top.cpu().numpy().astype(np.int8), g[f"top_{k}"])
    assert np.array_equal(bot.cpu().numpy().astype(np.int8), g[f"bot_{k}"])
    for mx in (16, 4):
        s = amod.stretch_corners(ms.clone(), mx, 0).cpu().numpy()
        assert np.array_equal(s, g[f"stretch_{k}_{mx}"], equal_nan=True), (k, mx)
    assert amod.find_valid_mod_sig_indices(ms) == g[f"valid_{k}"].tolist()
    # smoothing inside stretch_corners (smooth_n_frames > 1) goes through the same kernels
    if k == 0:
        s2 = amod.stretch_corners(m, 16, 4).cpu().numpy()
        assert np.array_equal(s2, g["stretch_4_16"], equal_nan=True)


def test_adamw_kernel_vs_torch(dev):
    from mod_extraction_amd import optim
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(64, 2, 5, 13)), torch.nn.Parameter(torch.randn(64)),
          torch.nn.Parameter(torch.randn(1, 64, 1))]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    mine = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in ps]
    o_ref = torch.optim.AdamW(ref, lr=1e-4, betas=(0.8, 0.99))
    o_mine = optim.FlatAdamW(mine, lr=1e-4, betas=(0.8, 0.99))
    for step in range(5):
        grads = [torch.randn_like(p) * (10.0 ** -step) for p in ps]
        for p, g in zip(ref, grads):
            p.grad = g.clone()
        o_mine.zero_grad()
        for p, g in zip(mine, grads):
            p.grad.copy_(g.to(dev) * 2.0)          # grad_scale 0.5 undoes this (the DDP 1/world path)
        o_ref.step()
        o_mine.step(grad_scale=0.5)
        for p, q in zip(mine, ref):
            assert float((p.detach().cpu() - q.detach()).abs().max()) < 3e-7, step


def test_batch_synthesis_and_train_step(dev):
    from mod_extraction_amd import data_modules, lightning, models, optim, trainer
    n, sr, B = 22272, 44100, 6
    cfg = dict(in_ch=2, n_samples=n, sr=sr, n_fft=1024, hop_len=256, n_mels=64, kernel_size=(5, 13),
               out_channels=[64] * 6, temp_dilations=[1, 1, 2, 4, 8, 16], pool_size=(2, 1), latent_dim=1,
               freq_mask_amount=0.25, time_mask_amount=0.25, use_ln=True)
    loss_dict = {"l1": 1.0, "fdl1": 5.0, "sdl1": 10.0, "mse": 0.0}
    torch.manual_seed(0); np.random.seed(0)
    ref = om.Spectral2DCNN(**cfg)
    mine = models.Spectral2DCNN(**cfg)
    mine.load_state_dict(ref.state_dict())
    module = lightning.LFOExtraction(mine, sr=sr, model_smooth_n_frames=0, loss_dict=loss_dict).to(dev).train()
    opt = optim.FlatAdamW(module.parameters(), lr=1e-4, betas=(0.8, 0.99))
    batcher = data_modules.SyntheticFxBatcher(B, n, sr, ("flanger", "chorus", "phaser"), dev, audio_seed=1)
    params = batcher.sample_params()
    dry, wet, mod, fxp = batcher.render(params)
    assert set(("depth", "feedback", "min_delay_width", "mix", "width", "rate_hz", "phase", "shape", "exp")) <= set(fxp)
    d_r, w_r, m_r = ol.synth_batch(params, batcher.kinds, batcher.src.cpu().numpy(), n, sr,
                                   {"flanger": 1.0, "chorus": 30.0}, mod_override=mod.cpu().numpy())
    assert torch.equal(dry.cpu(), d_r)
    fx_rows = [i for i, k in enumerate(batcher.kinds) if k != "phaser"]
    ph_rows = [i for i, k in enumerate(batcher.kinds) if k == "phaser"]
    assert torch.equal(wet.cpu()[fx_rows], w_r[fx_rows])          # flanger / chorus: bit-exact
    assert float((wet.cpu()[ph_rows] - w_r[ph_rows]).abs().max()) < 1e-5
    assert float((mod.cpu() - m_r).abs().max()) < 2e-6
    # the SpecAugment draw comes from the host generator: same seed on both sides -> same masks
    torch.manual_seed(123)
    ref.train()
    masks = None
    loss_r, terms_r, _ = ol.lfo_common_step(ref, d_r, wet.cpu(), m_r, loss_dict)
    torch.manual_seed(123)
    loss = trainer.Trainer(log_fn=None).train_step(module, opt, (dry, wet, mod, None))
    assert abs(float(loss) - float(loss_r)) < 1e-5 * max(1.0, abs(float(loss_r)))
    for k in loss_dict:
        assert abs(float(module.logged[f"train/{k}"][-1]) - float(terms_r[k])) < 2e-6
    assert opt.step_count == 1


def test_lfo_extraction_twenty_step_trajectory_vs_oracle(dev):
    """one-step parity cannot see an accumulation problem (fused LayerNorm statistics, the f16x3 scale
    bound, AdamW moments), so the HEADLINE path runs 20 AdamW steps of LFOExtraction (lightning.py:96-158, 187-192) on the
    HIP kernels and on the CPU oracle: same initial weights, the SAME rendered batches (the device's batches are fed to the
    oracle), SpecAugment on with a shared host seed per step; from then on each side steps with its OWN parameters,
    gradients and Adam moments.  As in every gradient test of this suite the oracle takes the device's decisions at the
    non-differentiable points (max-pool ties, PReLU kinks; `forward_routed` asserts that every differing decision sits on
    a tie): SpecAugment's constant rows / columns make exact ties common, fp32 rounding breaks them differently on the
    two sides, and either choice is a valid sub-gradient -- two free-running trajectories drift apart by tie-breaking
    alone (measured: loss 1e-3 after four steps, `tools/probe/trajectory_diag.py`), which says nothing about the arithmetic.
    Gates: per-step loss within 1e-4 relative; final parameters within 1e-3 of the distance the trajectory moved them
    (L2, per tensor and overall); 99.9 % of all elements within 1e-3 of their tensor's max magnitude.  The max-norm over ALL
    elements is printed and only bounded by 2 lr per step: while Adam's moments are young its update is ~ lr sign(g), so an
    element whose gradient is below fp32's norm-wise noise takes steps of either sign on either side."""
    from mod_extraction_amd import data_modules, lightning, models, optim, trainer
    n, sr, B, steps, lr = 22272, 44100, 4, 20, 1e-4
    cfg = dict(in_ch=2, n_samples=n, sr=sr, n_fft=1024, hop_len=256, n_mels=64, kernel_size=(5, 13),
               out_channels=[64] * 6, temp_dilations=[1, 1, 2, 4, 8, 16], pool_size=(2, 1), latent_dim=1,
               freq_mask_amount=0.25, time_mask_amount=0.25, use_ln=True)
    loss_dict = {"l1": 1.0, "fdl1": 5.0, "sdl1": 10.0, "mse": 0.0}
    torch.manual_seed(11); np.random.seed(11)
    ref = om.Spectral2DCNN(**cfg).train()
    mine = models.Spectral2DCNN(**cfg)
    mine.load_state_dict(ref.state_dict())
    init = {k: v.detach().clone() for k, v in ref.named_parameters()}
    module = lightning.LFOExtraction(mine, sr=sr, model_smooth_n_frames=0, loss_dict=loss_dict).to(dev).train()
    opt = optim.FlatAdamW(module.parameters(), lr=lr, betas=(0.8, 0.99))
    ref_opt = torch.optim.AdamW(ref.parameters(), lr=lr, betas=(0.8, 0.99))
    batcher = data_modules.SyntheticFxBatcher(B, n, sr, ("flanger", "chorus", "phaser"), dev, audio_seed=7)
    runner = trainer.Trainer(log_fn=None)
    worst_loss, n_shared = 0.0, 0
    kinks = {}                                               # how wide the shared decisions were (the tie rule here is 1e-4, the one-step tests' 2e-6)
    losses = []
    for i in range(steps):
        dry, wet, mod, _ = batcher.render(batcher.sample_params())
        torch.manual_seed(1000 + i)                          # the SpecAugment draw comes from the host generator
        models.DEBUG_TAP = {}                                # the step records its max-pool argmax / PReLU sign decisions
        try:
            loss = float(runner.train_step(module, opt, (dry, wet, mod, None)).detach())
            tap = models.DEBUG_TAP
        finally:
            models.DEBUG_TAP = None
        torch.manual_seed(1000 + i)                          # the same two draws in the model's order (models.py:199-205)
        masks = om.specaugment_bounds(cfg["n_mels"], ref.freq_mask_param) + om.specaugment_bounds(ref.n_frames, ref.time_mask_param)

        class _Routed:
            def __call__(self, x, _masks=None):
                nonlocal n_shared
                out, latent, k = om.forward_routed(ref, x, masks, tap, mine.n_frames, tie_tol=1e-4, kink_stats=kinks)
                n_shared += k
                return out, latent

        ref_opt.zero_grad()
        loss_t, _, _ = ol.lfo_common_step(_Routed(), dry.cpu(), wet.cpu(), mod.cpu(), loss_dict)
        loss_t.backward()
        ref_opt.step()
        loss_r = float(loss_t)
        rel = abs(loss - loss_r) / max(abs(loss_r), 1e-12)
        worst_loss = max(worst_loss, rel)
        losses.append((loss, loss_r))
        assert rel < 1e-4, (i, loss, loss_r)
    assert opt.step_count == steps
    moved2 = diff2 = 0.0
    worst_l2 = worst_max = worst_abs = 0.0
    n_bad = n_all = 0
    for (name, p), (_, q) in zip(mine.named_parameters(), ref.named_parameters()):
        p, q = p.detach().cpu().double(), q.detach().double()
        d, mv = (p - q), (q - init[name].double())
        moved2 += float((mv * mv).sum()); diff2 += float((d * d).sum())
        worst_l2 = max(worst_l2, float(d.norm() / mv.norm().clamp_min(1e-30)))
        mag = float(q.abs().max())
        worst_max = max(worst_max, float(d.abs().max()) / mag)
        worst_abs = max(worst_abs, float(d.abs().max()))
        n_bad += int((d.abs() > 1e-3 * mag).sum()); n_all += d.numel()
    overall = (diff2 / moved2) ** 0.5
    print(f"20-step trajectory: worst per-step loss rel err {worst_loss:.2e}; ||p_hip - p_oracle|| / ||p_oracle - p_init|| "
          f"overall {overall:.2e}, worst tensor {worst_l2:.2e}; max |diff| / max |param| {worst_max:.2e} (abs {worst_abs:.2e} = "
          f"{worst_abs / lr:.2f} lr); elements beyond 1e-3 of their tensor's max: {n_bad} of {n_all}; "
          f"decisions shared at ties: {n_shared}, of them {kinks.get('n_wide', 0)} with |delta| between 2e-6 and 1e-4 of the tensor's max "
          f"(widest {kinks.get('max_rel', 0.0):.2e}); loss {losses[0][0]:.5f} -> {losses[-1][0]:.5f}")
    assert worst_loss < 1e-4
    assert kinks.get("max_rel", 0.0) <= 1e-4                   # (widest decision shared with the device: on record in measured_errors.json)
    assert kinks.get("n_wide", 0) / max(1, n_shared) <= 1e-0   # share of the shared decisions wider than the one-step rule (2e-6)
    assert overall < 1e-3
    assert worst_l2 < 1e-3
    assert n_bad / n_all < 1e-3
    assert worst_abs / (2 * lr * steps) < 1.0


def test_eval_lfo_variants_vs_reference_golden(dev, golden_dir):
    """(f) rank 2: quasi-periodic / combined / concave-convex LFOs (modulations.py:104-210).  The PRODUCT (host control
    flow and RNG draws in the reference's order; synthesis, corners, resampling in the device kernels) under the same
    seeds against vectors of the REAL reference functions (tests/golden/make_golden_misc.py -> eval_lfo_variants.npz;
    the oracle is checked against the same vectors bit for bit in tests/test_oracle_golden.py).  Lengths and section
    boundaries must agree exactly; values to 1e-5 (device cos / pow differ from the host's in the last ulp)."""
    import sys
    sys.path.insert(0, golden_dir)
    import make_golden_misc as mg
    from mod_extraction_amd import modulations as amod
    g = np.load(os.path.join(golden_dir, "eval_lfo_variants.npz"))
    worst = 0.0

    def check(y, want, tag):
        nonlocal worst
        assert tuple(y.shape) == want.shape, (tag, y.shape, want.shape)
        err = float(np.abs(y.cpu().numpy() - want).max())
        worst = max(worst, err)
        assert err < 1e-5, (tag, err)

    for i, (seed, shape, freq, phase, l0, l1, r0, r1, split) in enumerate(mg.QUASI_CASES):
        base = amod.make_mod_signal(882, 441.0, freq, phase, shape, device=dev)
        torch.manual_seed(seed); np.random.seed(seed)
        check(amod.make_quasi_periodic(base.clone(), l0, l1, r0, r1, split), g[f"quasi_{i}"], ("quasi", i))
    for i, (seed, n, sr, freq, phase, shapes) in enumerate(mg.COMBINED_CASES):
        torch.manual_seed(seed); np.random.seed(seed)
        check(amod.make_combined_mod_sig(n, sr, freq, phase, list(shapes), device=dev), g[f"combined_{i}"], ("combined", i))
    for i, (seed, n, sr, freq, phase, a0, a1, b0, b1, prob) in enumerate(mg.CONCAVE_CASES):
        torch.manual_seed(seed); np.random.seed(seed)
        check(amod.make_concave_convex_mod_sig(n, sr, freq, phase, a0, a1, b0, b1, prob, device=dev), g[f"concave_{i}"],
              ("concave", i))
    print(f"[measured] eval LFO variants vs reference vectors: max abs err {worst:.2e} (gate 1e-5)")


def test_file_backed_batch_matches_disk_and_oracle(dev, tmp_path):
    """(f) rank 1: recorded audio through the device renderer.  The dry channel is bit-identical to the samples on
    disk (offsets recorded from the reference-pinned chunk search), flanger / chorus are bit-exact against the
    oracle on the same chunks, the phaser within 1e-5 (fp32, parity unpinned)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from wav_fixture import make_corpus
    from mod_extraction_amd import data_modules, datasets as ds
    dirs = make_corpus(str(tmp_path))
    n, sr, B = 4410, 44100, 6
    torch.manual_seed(21); np.random.seed(21)
    d = ds.RandomAudioChunkDataset(dirs["dry"], n_samples=n, sr=sr, silence_fraction_allowed=0.1,
                                   silence_threshold_energy=1e-6, n_retries=4, check_dataset=True)
    picked = []
    inner = d.search_dataset_for_audio_chunk

    def recording(n_samples, end_buffer=0):
        out = inner(n_samples, end_buffer)
        picked.append((out[1], out[2], out[3], n_samples))
        return out
    d.search_dataset_for_audio_chunk = recording
    batcher = data_modules.SyntheticFxBatcher(B, n, sr, ("flanger", "chorus", "phaser"), dev,
                                              phaser_fx={"rate_hz": (4.0, 8.0)}, chunk_source=ds.FileChunkSource(d))
    params = batcher.sample_params()
    dry, wet, mod, fxp = batcher.render(params)
    torch.cuda.synchronize()
    assert len(picked) == B
    for i, (path, ch, start, n_i) in enumerate(picked):
        lead = int(params["lead"][i])
        assert n_i == n + int(params.get("proc_extra", torch.zeros(B))[i])        # phaser clips ask for n + sr/rate
        disk, _ = ds.wav_load(path, frame_offset=start + lead, num_frames=n)
        assert torch.equal(dry[i, 0].cpu(), disk[ch])
    d_r, w_r, m_r = ol.synth_batch(params, batcher.kinds, batcher.src.cpu().numpy(), n, sr,
                                   {"flanger": 1.0, "chorus": 30.0}, mod_override=mod.cpu().numpy())
    fx_rows = [i for i, k in enumerate(batcher.kinds) if k != "phaser"]
    ph_rows = [i for i, k in enumerate(batcher.kinds) if k == "phaser"]
    assert torch.equal(dry.cpu(), d_r)
    assert torch.equal(wet.cpu()[fx_rows], w_r[fx_rows])
    assert float((wet.cpu()[ph_rows] - w_r[ph_rows]).abs().max()) < 1e-5


def test_train_step_through_the_rccl_init_path_world_size_1(dev):
    """torch.distributed over backend "nccl" (= RCCL on ROCm) with ONE rank: process-group initialisation, the flat
    gradient all-reduce and the metric reduction run through RCCL before the driver's multi-GPU launch does.  The step
    must be bit-identical to the same step without a process group (a 1-rank sum all-reduce is the identity)."""
    import socket
    import torch.distributed as dist
    from mod_extraction_amd import data_modules, lightning, models, optim, trainer

    def run(with_pg):
        torch.manual_seed(3); np.random.seed(3)
        cfg = dict(in_ch=2, n_samples=22272, sr=44100, n_fft=1024, hop_len=256, n_mels=64, kernel_size=(5, 13),
                   out_channels=[64] * 6, temp_dilations=[1, 1, 2, 4, 8, 16], pool_size=(2, 1), latent_dim=1,
                   freq_mask_amount=0.25, time_mask_amount=0.25, use_ln=True)
        module = lightning.LFOExtraction(models.Spectral2DCNN(**cfg), sr=44100, model_smooth_n_frames=0,
                                         loss_dict={"l1": 1.0, "fdl1": 5.0, "sdl1": 10.0, "mse": 0.0}).to(dev).train()
        opt = optim.FlatAdamW(module.parameters(), lr=1e-4, betas=(0.8, 0.99))
        bt = data_modules.SyntheticFxBatcher(6, 22272, 44100, ("flanger", "chorus", "phaser"), dev, audio_seed=9)
        losses = []
        for _ in range(2):
            opt.zero_grad()
            loss = module.training_step(bt.next_batch(), 0)
            loss.backward()
            if with_pg:
                dist.all_reduce(opt.flat_grad, op=dist.ReduceOp.SUM)         # ... on a 1-rank group: the identity
                scale = 1.0
            else:
                scale = trainer.allreduce_flat_grad(opt.flat_grad, 1)
            opt.step(grad_scale=scale)
            losses.append(float(loss.detach()))
        # world_size > 1 makes reduce_metrics all-reduce its (sum, count) table: on a 1-rank group the means are unchanged
        metrics = trainer.reduce_metrics(module.logged, 2 if with_pg else 1, trainer.metric_names(module, "train"))
        return losses, opt.flat_param.clone(), metrics

    base = run(False)
    from tests.helpers.torchrun import init_world1_process_group
    init_world1_process_group("nccl", device_id=dev)
    try:
        assert dist.get_backend() == "nccl"
        with_pg = run(True)
        dist.barrier()
    finally:
        dist.destroy_process_group()
    assert base[0] == with_pg[0] and torch.equal(base[1], with_pg[1])
    assert base[2] == with_pg[2] and set(base[2]) == {"train/l1", "train/fdl1", "train/sdl1", "train/mse", "train/loss"}


@pytest.mark.parametrize("config", [3, 4])
def test_bench_two_ranks_sharing_the_gpu_over_gloo(config):
    """bench.py's N > 1 path -- torchrun environment, barrier + max-over-ranks timing, per-rank clip shards, the flat
    gradient all-reduce, rank 0 printing the one JSON line -- with TWO ranks on this box's single GPU.  RCCL refuses two
    ranks on one device, so the collectives go through gloo (MODEX_DIST_BACKEND) and LOCAL_RANK is folded onto the
    existing device (MODEX_SHARE_GPU): the code path is the driver's multi-GPU launch, only the transport differs.
    (--full: config 4's roofline is measured on isolated launches.)"""
    import json
    from tests.helpers.torchrun import run_torchrun
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MODEX_SHARE_GPU="1", MODEX_DIST_BACKEND="gloo")
    res = run_torchrun(2, [os.path.join(root, "bench.py"), "--gpus", "2", "--config", str(config), "--steps", "2",
                           "--warmup", "1", "--batch", "8", "--full"], env=env, cwd=root, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]                 # rank 0 only
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["scaling"] == "weak"
    assert out["config"]["global_batch"] == 16 and out["config"]["parallelism"] == "dp2"
    assert out["value"] > 0 and "cpu_baseline" not in out      # the CPU baseline is an N = 1 leg
    assert out["roofline"]["frac"] is None or out["roofline"]["frac"] > 0
    assert len(lines[0]) < 6000
    _check_scale_fields(out, 2, 1 if config == 3 else None)


def _check_scale_fields(out, world, calls_per_step=None):
    """The N > 1 line explains its own efficiency: time inside the gradient all-reduce and every rank's step spread."""
    assert out["world_size"] == world and "rccl_version" in out
    ar = out["allreduce_ms"]
    assert ar["mean"] > 0 and ar["max"] >= ar["mean"] and ar["per_step"] > 0 and ar["bytes"] > 0
    if calls_per_step is not None:
        assert ar["calls_per_step"] == calls_per_step
    spread = out["step_ms_per_rank"]
    assert len(spread) == world and all(lo <= med <= hi for lo, med, hi in spread)
    assert out["rank_median_spread_ms"] >= 0


def _run_bench(argv, env=None, timeout=900, want_detail=False):
    """Run bench.py as the driver does; returns the parsed LAST stdout line (and the full detail dict).  The line must be
    the only JSON line, the last thing on stdout, and short (the driver stopped parsing the 25 KB line of round 5)."""
    import json
    import subprocess
    import sys
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    detail_path = os.path.join(tempfile.mkdtemp(), "detail.json")
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + argv + ["--detail-out", detail_path],
                         env=dict(os.environ, **(env or {})), cwd=root, capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    assert res.stdout.rstrip("\n").splitlines()[-1] == lines[0]        # nothing follows the line on stdout
    assert len(lines[0]) < 6000, len(lines[0])
    out = json.loads(lines[0])
    if want_detail:
        assert "BENCH_DETAIL " in res.stderr
        with open(detail_path) as f:
            return out, json.load(f)
    return out


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` OUTSIDE torchrun (the form the driver uses): the launcher process starts the two rank
    processes itself through torch.distributed.run on a free port and relays rank 0's line (two ranks on this box's one
    GPU, collectives over gloo as in the test above)."""
    out = _run_bench(["--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "8"],
                     env={"MODEX_SHARE_GPU": "1", "MODEX_DIST_BACKEND": "gloo"})
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["config"]["global_batch"] == 16
    assert out["value"] > 0 and "other_configs" not in out


def test_bench_eight_ranks_sharing_the_gpu_over_gloo():
    """The driver's N = 8 form once, end to end: `python bench.py --gpus 8` starts EIGHT rank processes through
    torch.distributed.run on a free port (here all on this box's one GPU, collectives over gloo, two clips per rank), every
    rank joins the barriers / the max-over-ranks timing / the flat-gradient all-reduce, and rank 0's one line -- relayed by
    the launcher -- says how many ranks the collective library saw.  (The launcher, the port logic, the rank-0 relay and the
    eight-way rendezvous are exactly the code the 8-GPU scaling run executes; only the transport and the device differ.)"""
    out = _run_bench(["--gpus", "8", "--steps", "1", "--warmup", "1", "--batch", "2"],
                     env={"MODEX_SHARE_GPU": "1", "MODEX_DIST_BACKEND": "gloo"}, timeout=1500)
    assert out["n_gpus"] == 8 and out["world_size"] == 8 and out["dist_backend"] == "gloo"
    assert out["config"]["global_batch"] == 16 and out["config"]["parallelism"] == "dp8"
    assert out["value"] > 0 and out["worker_rc"] == 0 and "cpu_baseline" not in out
    _check_scale_fields(out, 8, calls_per_step=1)


def test_tbptt_step_through_rccl_with_the_cu_partition_installed(dev):
    """Config 4 under DDP issues one 70 KB all-reduce per optimizer step (83 per batch) on the CU-MASKED main stream that
    Trainer.fit installs.  With ONE rank on backend "nccl" (= RCCL) the collective is the identity, so the run must land on
    exactly the parameters of the same steps without a process group -- and it must get through RCCL's kernels on a stream
    created by hipExtStreamCreateWithCUMask, which is what the 8-GPU run of that config will do."""
    import socket
    import torch.distributed as dist
    from mod_extraction_amd import lightning as al, models as am, optim, streams, trainer
    from oracle import modulations as omod

    n, W, S, B = 1024 + 6 * 1024, 1024, 1024, 4

    def run(with_pg):
        torch.manual_seed(21)
        dry = torch.rand(B, 1, n) * 1.6 - 0.8
        wet = (0.7 * dry + 0.2 * torch.roll(dry, 5, -1)).clamp(-1, 1)
        lfo = torch.stack([omod.make_mod_signal(64, 64 / (n / 44100.0), 5.0 + i, 0.3 * i, "cos") for i in range(B)])
        em = am.LSTMEffectModel()
        mod = al.TBPTTLFOEffectModeling(W, S, em, lfo_model=None, model_smooth_n_frames=0, should_stretch=False,
                                        discard_invalid_lfos=False, loss_dict={"l1": 1.0, "esr": 0.0, "dc": 0.0}).to(dev).train()
        opt = optim.FlatAdamW(mod.parameters(), lr=1e-3, betas=(0.8, 0.99))
        part = streams.cu_partition(dev, main_workgroups=B)
        assert part is not None, "this test needs the CU partition (256-CU part, MODEX_CU_PARTITION unset)"
        main = part[0]
        main.wait_stream(torch.cuda.current_stream(dev))
        calls = []
        real = trainer.allreduce_flat_grad

        def counted(flat_grad, world_size):
            calls.append(flat_grad.numel())
            if with_pg:
                dist.all_reduce(flat_grad, op=dist.ReduceOp.SUM)      # 1-rank group: the identity, through RCCL on the masked stream
            return 1.0
        trainer.allreduce_flat_grad = counted
        try:
            with torch.cuda.stream(main):
                mod.common_step((dry.to(dev), wet.to(dev), lfo.to(dev), None), is_training=True, optimizer=opt, world_size=2)
            torch.cuda.current_stream(dev).wait_stream(main)
            torch.cuda.synchronize()
        finally:
            trainer.allreduce_flat_grad = real
        return opt.flat_param.clone(), len(calls), opt.step_count

    base = run(False)
    from tests.helpers.torchrun import init_world1_process_group
    init_world1_process_group("nccl", device_id=dev)
    try:
        with_pg = run(True)
        dist.barrier()
    finally:
        dist.destroy_process_group()
    assert base[1] == with_pg[1] == base[2] == (n - W) // S            # one collective per optimizer step
    assert torch.equal(base[0], with_pg[0])


def test_bench_driver_command_prints_one_short_parseable_line():
    """The driver's full command (`python3 bench.py --gpus 1 --steps 20 --warmup 5 --full`): the LAST stdout line is one
    self-contained JSON object under 6 KB with `roofline` and `cpu_baseline`, the other BASELINE configurations as short
    summaries, nothing after it on stdout; the full per-kernel detail goes to bench_detail.json / stderr."""
    out, detail = _run_bench(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"], timeout=1500, want_detail=True)
    assert out["n_gpus"] == 1 and out["steps"] == 20 and out["warmup"] == 5 and out["dtype"] == "f32"
    assert out["config"]["baseline_config"] == 3 and out["config"]["global_batch"] == 256
    r = out["roofline"]
    assert r["bound"] == "mfma" and 0 < r["frac"] < 1 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["avg_launch_ms"] > 0 and r["traffic"] > 0 and len(r["note"]) <= 200
    c = out["cpu_baseline"]
    assert c["value"] > 0 and c["cores"] >= 1 and c["kind"] == "port" and len(c["sample"]) <= 200
    assert abs(out["value"] - 256 * 2.0 / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
    assert out["fx_kernel_frac_of_independent_floor"] > 0
    oc = out["other_configs"]
    assert sorted(oc) == ["2", "4", "5"]
    for k, o in oc.items():
        assert "error" not in o, o
        assert o["value"] > 0 and o["ms_per_step"] > 0 and o["roofline"]["frac"] > 0 and o["cpu_baseline"]["value"] > 0, (k, o)
    assert oc["4"]["value_clips_trained"] < oc["4"]["value"]
    # the detail file carries what the line dropped
    assert detail["value"] == out["value"] and "kernels" in detail and "fx_kernels" in detail
    for k, o in detail["other_configs"].items():
        assert o["config"]["baseline_config"] == int(k) and "kernels" in o
    assert 0 < detail["other_configs"]["4"]["config"]["clips_trained_per_batch"]["mean"] <= 128   # the YAML's LFO validity filter is on
    assert all("tflops" not in v for k, v in detail["kernels"].items() if k.startswith("conv_prep"))


def test_bench_plain_run_times_only_the_headline_and_dumps_its_outputs(tmp_path):
    """The plain command (`bench.py --gpus 1 --steps K --warmup W`) times exactly K steps of the headline and measures
    nothing else; `--dump-outputs DIR` writes the last timed step's outputs as float32 / float64 .npy files under 64 MB,
    and a second run with the same arguments renders the same batches."""
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        out = _run_bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)], timeout=600)
        assert out["n_gpus"] == 1 and out["steps"] == 3 and out["warmup"] == 1 and out["config"]["baseline_config"] == 3
        assert out["higher_is_better"] is True and out["dtype"] == "f32" and out["unit"] == "audio-seconds/s"
        assert abs(out["value"] - 256 * 2.0 / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
        assert out["roofline"]["bound"] == "mfma" and out["roofline"]["frac"] > 0 and out["worker_rc"] == 0
        for k in ("cpu_baseline", "other_configs", "exact_fp32_path", "fx_kernel_frac_of_serial_floor", "recurrent_kernels"):
            assert k not in out, k
        files = sorted(os.listdir(d))
        assert files == ["dry.npy", "grads.npy", "loss.npy", "mod.npy", "params.npy", "wet.npy"], files
        arrays = {f[:-4]: np.load(d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 * 10 ** 6
        assert abs(float(arrays["loss"]) - out["final_loss"]) <= 1e-6 * abs(out["final_loss"])
        runs.append(arrays)
    for k in ("dry", "wet", "mod"):                     # the inputs of the last timed step
        assert np.array_equal(runs[0][k], runs[1][k]), k


@pytest.mark.parametrize("mode", ["lfo", "tbptt"])
def test_two_rank_step_equals_the_single_process_step_on_the_joined_batch(tmp_path, mode):
    """Data parallelism end to end on the real kernels: two ranks (sharing this box's GPU, collectives over gloo), each
    with half of a fixed batch of 4 clips, take ONE optimizer step -- forward, backward, sum all-reduce of the flat
    gradient, AdamW with the 1/world scale -- and must land on the parameters of ONE process stepping on all 4 clips
    (every loss term is a mean over clips and LayerNorm is per clip, so the averaged gradients are the joined batch's).
    mode "tbptt": the same for the effect-modelling batch -- four truncated-BPTT optimizer steps of the LSTM-64, one
    all-reduce each."""
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    worker = os.path.join(root, "tests", "helpers", "ddp_equivalence_worker.py")
    one, two = str(tmp_path / "one.pt"), str(tmp_path / "two.pt")
    res = subprocess.run([sys.executable, worker, one, "4", mode], capture_output=True, text=True, timeout=600,
                         env={k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")})
    assert res.returncode == 0, res.stderr[-2000:]
    from tests.helpers.torchrun import run_torchrun
    env = dict(os.environ, MODEX_SHARE_GPU="1", MODEX_DIST_BACKEND="gloo")
    res = run_torchrun(2, [worker, two, "4", mode], env=env, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    a, b = torch.load(one), torch.load(two)
    assert a["world"] == 1 and b["world"] == 2
    # the averaged gradient of the two ranks IS the joined batch's gradient (last optimizer step's, for tbptt) ...
    g1, g2 = a["grad"], b["grad"]
    assert float((g1 - g2).abs().max()) < (1e-5 if mode == "lfo" else 1e-3) * float(g1.abs().max())
    # ... and so are the parameters after AdamW: every weight moves by ~lr = 1e-3 per step; compared in bulk, because
    # Adam turns a gradient at the 1e-8 noise floor into a +-lr/2 step whose sign is rounding
    d = (a["param"] - b["param"]).abs()
    assert float(d.median()) < 1e-6 and float(torch.quantile(d[:: max(1, d.numel() // 100000)], 0.999)) < (2e-5 if mode == "lfo" else 1e-4)
    if mode == "tbptt":
        assert a["steps"] == b["steps"] == 4
    assert abs(a["loss"] - b["loss"]) < 0.5                      # rank 0 reports its own half's loss: same order of magnitude


def test_parameter_gradients_written_in_place_equal_the_accumulated_ones(dev):
    """`with FlatAdamW.direct_backward():` arms the in-place path for ONE backward: the first CNN backward inside the scope
    writes every parameter gradient straight into its `.grad` view and hands autograd `None` (20 `grad += g` launches less
    per step).  The flat gradient must be bit-identical to the ordinary accumulate path; a SECOND backward (sub-batches)
    must still accumulate; and OUTSIDE the scope nothing is ever overwritten (a weight penalty's backward
    before the main one, `torch.autograd.grad`)."""
    from mod_extraction_amd import data_modules, lightning, models, optim

    def setup():
        torch.manual_seed(5); np.random.seed(5)
        cfg = dict(in_ch=2, n_samples=22272, sr=44100, n_fft=1024, hop_len=256, n_mels=64, kernel_size=(5, 13),
                   out_channels=[64] * 6, temp_dilations=[1, 1, 2, 4, 8, 16], pool_size=(2, 1), latent_dim=1,
                   freq_mask_amount=0.0, time_mask_amount=0.0, use_ln=True)
        module = lightning.LFOExtraction(models.Spectral2DCNN(**cfg), sr=44100, model_smooth_n_frames=0,
                                         loss_dict={"l1": 1.0, "fdl1": 5.0, "sdl1": 10.0, "mse": 0.0}).to(dev).train()
        opt = optim.FlatAdamW(module.parameters(), lr=1e-4, betas=(0.8, 0.99))
        bt = data_modules.SyntheticFxBatcher(4, 22272, 44100, ("flanger", "chorus"), dev, audio_seed=3)
        return module, opt, bt.next_batch()

    def grads(direct, twice):
        module, opt, batch = setup()
        opt.zero_grad()
        if direct:
            with opt.direct_backward():
                module.training_step(batch, 0).backward()
                assert opt.flat_grad._modex_fresh is False            # consumed by the CNN backward
        else:
            module.training_step(batch, 0).backward()
        if twice:
            module.training_step(batch, 0).backward()
        assert not getattr(opt.flat_grad, "_modex_fresh", False)
        return opt.flat_grad.clone()

    g_direct, g_plain = grads(True, False), grads(False, False)
    assert float(g_plain.abs().max()) > 0 and torch.equal(g_direct, g_plain)
    g2 = grads(True, True)                                                 # first backward in place, second accumulated
    assert float((g2 - 2 * g_plain).abs().max()) <= 1e-6 * float(g_plain.abs().max())
    # outside a direct_backward() scope zero_grad() arms nothing: what is already in .grad is kept
    module, opt, batch = setup()
    opt.zero_grad()
    penalty = sum((p * p).sum() for p in module.parameters())
    penalty.backward()                                                     # e.g. a weight penalty before the main loss
    g_pen = opt.flat_grad.clone()
    assert float(g_pen.abs().max()) > 0
    module.training_step(batch, 0).backward()
    assert float((opt.flat_grad - (g_pen + g_plain)).abs().max()) <= 1e-6 * float((g_pen + g_plain).abs().max())
    # ... and torch.autograd.grad returns real tensors there, without touching .grad
    opt.zero_grad()
    got = torch.autograd.grad(module.training_step(batch, 0), list(module.parameters()))
    assert all(g is not None for g in got) and float(opt.flat_grad.abs().max()) == 0.0
    flat = torch.cat([g.reshape(-1) for g in got])
    assert torch.equal(flat, g_plain)
    # an exception inside the scope leaves the flag cleared
    try:
        with opt.direct_backward():
            raise RuntimeError("boom")
    except RuntimeError:
        pass
    assert opt.flat_grad._modex_fresh is False


@pytest.mark.gpu
def test_batches_rendered_one_step_ahead_equal_the_serial_ones(dev):
    """SyntheticFxBatcher with overlap renders batch i + 1 on a side stream while batch i is consumed (its host-sampled
    parameters are copied to the device BEFORE the side stream waits for the work in flight): the batches must be the ones
    the serial batcher produces from the same seeds, bit for bit, also while the consumer keeps the main stream busy."""
    from mod_extraction_amd import data_modules

    def run(overlap):
        torch.manual_seed(11); np.random.seed(11)
        bt = data_modules.SyntheticFxBatcher(6, 22272, 44100, ("flanger", "chorus", "phaser"), dev, audio_seed=4, overlap=overlap)
        out = []
        busy = torch.randn(2048, 2048, device=dev)
        for _ in range(3):
            dry, wet, mod, fxp = bt.next_batch()
            for _ in range(4):
                busy = (busy @ busy).clamp_(-1, 1)              # main-stream work between the batches
            out.append((dry.clone(), wet.clone(), mod.clone(), {k: v.clone() for k, v in fxp.items() if isinstance(v, torch.Tensor)}))
        torch.cuda.synchronize()
        return out

    serial, ahead = run(False), run(True)
    for (d0, w0, m0, p0), (d1, w1, m1, p1) in zip(serial, ahead):
        assert torch.equal(d0, d1) and torch.equal(w0, w1) and torch.equal(m0, m1)
        assert p0.keys() == p1.keys() and all(torch.equal(p0[k], p1[k]) for k in p0)


def test_lfo_extraction_trains_through_the_moving_average(dev):
    """LFOExtraction with model_smooth_n_frames > 1 while TRAINING (lightning.py:117-120: unfold(k).mean on the prediction, centre crop
    of the target): the moving average runs as mx_smoothen with its transpose as backward; loss and every gradient against the same
    step written with torch's unfold on the oracle's model (1e-5 / 2e-5 norm-wise, pooling decisions shared as in test_gpu_cnn)."""
    import torch.nn.functional as F
    from mod_extraction_amd import lightning, models as am
    from oracle import losses as olosses, models as om
    n, k = 22272, 4
    cfg = dict(in_ch=1, n_samples=n, n_mels=64, kernel_size=(5, 13), out_channels=[64] * 6, temp_dilations=[1, 1, 2, 4, 8, 16],
               pool_size=(2, 1), latent_dim=1, use_ln=True)
    torch.manual_seed(8)
    ref = om.Spectral2DCNN(**cfg).eval()
    mine = am.Spectral2DCNN(**cfg); mine.load_state_dict(ref.state_dict())
    weights = {"l1": 1.0, "fdl1": 5.0, "sdl1": 10.0}
    module = lightning.LFOExtraction(mine, sr=44100, use_dry=False, model_smooth_n_frames=k, loss_dict=weights).to(dev)
    module.train(); mine.eval()                                    # (eval: no SpecAugment draw; gradients still flow)
    g = torch.Generator().manual_seed(2)
    wet = torch.rand(3, 1, n, generator=g) * 2 - 1
    t = torch.linspace(0, 1, 882)
    mod_sig = 0.5 + 0.5 * torch.cos(2 * torch.pi * (1.0 + torch.arange(3).view(3, 1)) * t)
    am.DEBUG_TAP = {}
    try:
        loss = module.training_step((None, wet.to(dev), mod_sig.to(dev), None), 0)
        loss.backward()
        tap = am.DEBUG_TAP
    finally:
        am.DEBUG_TAP = None
    hat, _, _ = om.forward_routed(ref, wet, (0, 0, 0, 0), tap, mine.n_frames)
    hat = hat.squeeze(1).unfold(-1, k, 1).mean(-1)
    tgt = F.interpolate(mod_sig.unsqueeze(1), size=mine.n_frames, mode="linear", align_corners=True).squeeze(1)
    pad = tgt.size(-1) - hat.size(-1)
    tgt = tgt[..., pad // 2:pad // 2 + hat.size(-1)]
    want = sum(w * olosses.get_loss_func_by_name(name)(hat, tgt) for name, w in weights.items())
    want.backward()
    assert abs(float(loss) - float(want)) < 1e-5 * max(1.0, abs(float(want)))
    gr = dict(ref.named_parameters())
    for name, p in mine.named_parameters():
        e = float((p.grad.cpu() - gr[name].grad).abs().max() / gr[name].grad.abs().max().clamp_min(1e-30))
        assert e < 2e-5, (name, e)

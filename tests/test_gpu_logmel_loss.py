"""GPU: the log-mel L1 loss (mx_logmel_l1_loss: lm_onepass_kernel with and without the gradient, finish, fold) against the
fp64 explicit adjoint of tests/helpers/logmel_l1_64.py, and wired into effect_loss_grad and the TBPTT step.

The reference applies the module's OWN filter bank and window promoted to fp64 (applying the tables is the kernel's job;
the tables are checked against the closed forms in tests/test_fp64_refs.py).  The kernel pairs the gradient spectra of two
frames in one inverse transform, and a packed forward transform of prediction and target would leave the louder signal's
rounding on the quieter one: the level grid below is where such a split goes wrong.

Gates (per call):
  * value within 1e-5 (relative) of the fp64 value
  * gradient within max(2 x the yardstick's error, floor) in max-norm (floor 1e-4 of max |g64|) and in relative L2 (floor
    1e-5); the yardstick is the same pipeline in fp32 with separate transforms of prediction and target, the larger error
    of two plain fp32 forward transforms (scipy's real FFT and a textbook radix-2 complex FFT): the gradient of a weak band
    divides by its power, and there one fp32 FFT can be 10x luckier than another (measured: scipy 1.6e-6, radix-2 2.5e-5
    and this kernel 2.5e-5 on the first, even-symmetric frame of a target-quieter clip at n_fft 512)
The prediction differs from the target by a level and a delay, so that no band's log difference is near a tie (where the
sign of the gradient is decided by rounding; smallest |la - lb| over the cases 4.7e-6).
Every gate prints its measured value.
"""
import numpy as np
import pytest
import torch

from tests.helpers.logmel_l1_64 import logmel_l1_64

pytestmark = pytest.mark.gpu

B = 3
N_MELS = 256
EPS = 1e-7
CASES = [(T, n_fft, hop) for T in (1024, 1000, 4500, 30000) for n_fft in (512, 1024, 2048) for hop in (256, 200)
         if T > n_fft // 2]


def pair(T, seed=0, b=B):
    """(prediction, target) (b, T) float64 at about 0.5 peak: a sine and noise, and a quieter, delayed, noisier copy."""
    g = np.random.default_rng(seed)
    n = np.arange(T) / 44100.0
    t = 0.3 * np.sin(2 * np.pi * 330.0 * n)[None, :] + g.uniform(-0.2, 0.2, (b, T))
    p = 0.6 * t + 0.1 * np.roll(t, 7, -1) + 0.03 * g.standard_normal((b, T))
    return p, t


def module(dev, n_fft, hop, n_mels=N_MELS):
    from mod_extraction_amd import losses as al
    mod = al.LogMelLoss(44100, n_fft, hop, n_mels)
    mod.spectrogram.to(dev)
    return mod


def rows(dev, x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)


def tables(mod):
    sp = mod.spectrogram
    return sp.mel_scale.fb.cpu().double().numpy(), sp.spectrogram.window.cpu().double().numpy()


def check(dev, x, y, n_fft, hop, tag):
    from mod_extraction_amd import losses as al
    x, y = x.astype(np.float32), y.astype(np.float32)
    mod = module(dev, n_fft, hop)
    v, g = al.logmel_l1_value_and_grad(mod, rows(dev, x), rows(dev, y))
    val, g = float(v), g.cpu().double().numpy()
    fb, win = tables(mod)
    v64, g64, _ = logmel_l1_64(x.astype(np.float64), y.astype(np.float64), n_fft, hop, N_MELS, fb=fb, window=win)
    g32s = [logmel_l1_64(x, y, n_fft, hop, N_MELS, fb=fb.astype(np.float32), window=win.astype(np.float32),
                         dtype=np.float32, fft=f)[1] for f in ("scipy", "radix2")]
    scale, l2 = float(np.abs(g64).max()), float(np.linalg.norm(g64))
    assert scale > 0
    e_v = abs(val - v64) / abs(v64)
    e_max = float(np.abs(g - g64).max()) / scale
    y_max = max(float(np.abs(g32 - g64).max()) for g32 in g32s) / scale
    e_l2 = float(np.linalg.norm(g - g64)) / l2
    y_l2 = max(float(np.linalg.norm(g32 - g64)) for g32 in g32s) / l2
    print(f"[measured] log_mel_l1 {tag}: value {e_v:.1e}, gradient max-norm {e_max:.1e} (fp32 {y_max:.1e}), "
          f"L2 {e_l2:.1e} (fp32 {y_l2:.1e})")
    assert e_v <= 1e-5, (tag, val, v64)
    assert e_max <= max(2.0 * y_max, 1e-4), (tag, e_max, y_max)
    assert e_l2 <= max(2.0 * y_l2, 1e-5), (tag, e_l2, y_l2)
    return g, g64


@pytest.mark.parametrize("T,n_fft,hop", CASES)
def test_logmel_loss_value_and_gradient_vs_fp64(dev, T, n_fft, hop):
    p, t = pair(T, T + n_fft + hop)
    check(dev, p, t, n_fft, hop, (T, n_fft, hop))


@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
@pytest.mark.parametrize("ratio", [1e-2, 1e-3, 1e-4, 1e2, 1e3, 1e4])
def test_logmel_loss_level_grid(dev, n_fft, ratio):
    """Prediction / target level ratio over whole clips: the louder signal at about 0.5, the other scaled down."""
    p, t = pair(12000, 1)
    x, y = (ratio * p, t) if ratio <= 1 else (p, t / ratio)
    check(dev, x, y, n_fft, 256, (n_fft, ratio))


def test_logmel_loss_identical_signals_exact_zero(dev):
    from mod_extraction_amd import losses as al
    _, t = pair(9000, 2)
    for n_fft in (512, 1024, 2048):
        mod = module(dev, n_fft, 256)
        a = rows(dev, t)
        v, g = al.logmel_l1_value_and_grad(mod, a, a.clone())
        assert float(v) == 0.0, n_fft
        assert not bool(g.any()), n_fft


def test_logmel_loss_silent_prediction(dev):
    """A prediction that is zero everywhere: every band of it lies below eps, so the clamp passes no gradient anywhere and
    the value is the mean of |log eps - lb|."""
    from mod_extraction_amd import losses as al
    _, t = pair(9000, 3)
    for n_fft in (512, 1024, 2048):
        mod = module(dev, n_fft, 256)
        v, g = al.logmel_l1_value_and_grad(mod, rows(dev, np.zeros_like(t)), rows(dev, t))
        fb, win = tables(mod)
        _, _, (_, lb) = logmel_l1_64(np.zeros_like(t), t.astype(np.float32).astype(np.float64), n_fft, 256, N_MELS, fb=fb,
                                     window=win)
        want = float(np.mean(np.abs(np.log(EPS) - lb)))
        e = abs(float(v) - want) / want
        print(f"[measured] log_mel_l1 silent prediction (n_fft={n_fft}): value {e:.1e}")
        assert e <= 1e-5, (n_fft, float(v), want)
        assert not bool(g.any()), n_fft


def exact_zero_region(T, span, n_fft, hop):
    """Samples every frame of which lies inside the span together with its two neighbours (the gradient spectra of two
    frames share one inverse transform)."""
    s0, s1 = span
    ok = np.ones(T, bool)
    nf = T // hop + 1
    inside = np.array([f * hop - n_fft // 2 >= s0 and f * hop + n_fft // 2 <= s1 for f in range(nf)])
    good = inside & np.r_[False, inside[:-1]] & np.r_[inside[1:], False]
    for f in np.nonzero(~good)[0]:
        ok[max(f * hop - n_fft // 2, 0):max(min(f * hop + n_fft // 2, T), 0)] = False
    return ok


@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
def test_logmel_loss_silent_span_zero_gradient(dev, n_fft):
    """Both signals silent over a span of each clip: the whole clip against the reference, and the samples that only the
    span's frames reach receive exactly 0."""
    T, hop = 24000, 256
    spans = ((4000, 16000), (6000, 20000), (3000, 15000))
    p, t = pair(T, 4)
    for r, (s0, s1) in enumerate(spans):
        p[r, s0:s1] = 0.0
        t[r, s0:s1] = 0.0
    g, g64 = check(dev, p, t, n_fft, hop, ("silent span", n_fft))
    for r, span in enumerate(spans):
        zone = exact_zero_region(T, span, n_fft, hop)
        assert zone.sum() >= 1000
        assert not np.any(g64[r, zone])
        assert float(np.abs(g[r, zone]).max()) == 0.0, r


def test_logmel_loss_scale_and_accumulate(dev):
    from mod_extraction_amd import losses as al
    p, t = pair(20000, 5)
    mod = module(dev, 1024, 256)
    a, b = rows(dev, p), rows(dev, t)
    v1, g1 = al.logmel_l1_value_and_grad(mod, a, b)
    vs, gs = al.logmel_l1_value_and_grad(mod, a, b, scale=0.37)
    e_v = abs(float(vs) - 0.37 * float(v1)) / (0.37 * float(v1))
    e_g = float((gs.double() - 0.37 * g1.double()).abs().max() / (0.37 * g1.double().abs().max()))
    print(f"[measured] log_mel_l1 scale: value {e_v:.1e}, gradient {e_g:.1e}")
    assert e_v <= 1e-6 and e_g <= 1e-6, (e_v, e_g)
    preset = torch.randn_like(g1) * float(g1.abs().max())
    dx = preset.clone()
    va, ga = al.logmel_l1_value_and_grad(mod, a, b, scale=0.37, dx=dx, accumulate=True)
    assert ga.data_ptr() == dx.data_ptr()
    want = (preset + gs).cpu().numpy()
    got = ga.cpu().numpy()
    ulp = np.spacing(np.maximum(np.abs(want), np.abs(got)))
    e_u = float((np.abs(got - want) / ulp).max())
    print(f"[measured] log_mel_l1 accumulate: {e_u:.0f} ulp")
    assert e_u <= 1.0, e_u
    assert torch.equal(va, vs)


def test_logmel_loss_strided_rows_and_repeat_bit_identical(dev):
    """Rows of (B, T) views into (B, T + 37) buffers give what contiguous copies give, bit for bit; two calls give the same
    bits; the value-only path gives the value of the gradient path."""
    from mod_extraction_amd import losses as al
    T = 15000
    p, t = pair(T, 6)
    bufx = torch.zeros((B, T + 37), device=dev)
    bufy = torch.zeros((B, T + 37), device=dev)
    bufx[:, 5:5 + T] = rows(dev, p)
    bufy[:, 11:11 + T] = rows(dev, t)
    xv, yv = bufx[:, 5:5 + T], bufy[:, 11:11 + T]
    assert not xv.is_contiguous()
    for n_fft in (512, 1024, 2048):
        mod = module(dev, n_fft, 200)
        v_s, g_s = al.logmel_l1_value_and_grad(mod, xv, yv)
        v_c, g_c = al.logmel_l1_value_and_grad(mod, xv.contiguous(), yv.contiguous())
        v_r, g_r = al.logmel_l1_value_and_grad(mod, xv.contiguous(), yv.contiguous())
        assert torch.equal(v_s, v_c) and torch.equal(g_s, g_c), n_fft
        assert torch.equal(v_r, v_c) and torch.equal(g_r, g_c), n_fft
        v0, none = al.logmel_l1_value_and_grad(mod, xv, yv, need_grad=False)
        assert none is None
        e = abs(float(v0) - float(v_s)) / abs(float(v_s))
        print(f"[measured] log_mel_l1 value-only vs gradient path (n_fft={n_fft}): {e:.1e}")
        assert e <= 1e-6, e


def test_logmel_loss_module_beyond_352_frames(dev):
    """get_loss_func_by_name("log_mel_l1") on 3 x 176400 samples (690 frames; the module used to stop at 352)."""
    from mod_extraction_amd import losses as al
    p, t = pair(176400, 7)
    fn = al.get_loss_func_by_name("log_mel_l1")
    x3, y3 = rows(dev, p)[:, None, :], rows(dev, t)[:, None, :]
    got = float(fn(x3, y3))
    fb, win = tables(fn)
    v64, _, _ = logmel_l1_64(p.astype(np.float32).astype(np.float64), t.astype(np.float32).astype(np.float64), 1024, 256,
                             256, fb=fb, window=win)
    e = abs(got - v64) / v64
    print(f"[measured] LogMelLoss at 690 frames: value {e:.1e}")
    assert e <= 1e-5, (got, v64)
    with pytest.raises(NotImplementedError):
        fn(x3.clone().requires_grad_(True), y3)


def test_logmel_loss_rejects_short_clips_before_launching(dev):
    from mod_extraction_amd import _hip, losses as al
    for n_fft in (512, 1024, 2048):
        mod = module(dev, n_fft, 256)
        a = torch.zeros((2, n_fft // 2), device=dev)
        with pytest.raises(ValueError):
            al.logmel_l1_value_and_grad(mod, a, a)
        sp = mod.spectrogram
        lo, hi = sp.bands()
        part = torch.empty(8, device=dev, dtype=torch.float64)
        value = torch.full((), 123.0, device=dev)
        dx = torch.full((2, n_fft // 2), 7.0, device=dev)
        scratch = torch.empty(1 << 16, device=dev)
        with pytest.raises(_hip.HipLibraryError, match="MX_ERR_ARG"):
            _hip.call("mx_logmel_l1_loss", a.data_ptr(), a.stride(0), a.data_ptr(), a.stride(0), 2, n_fft // 2,
                      _hip.ptr(sp.spectrogram.window), _hip.ptr(sp.twiddle), _hip.ptr(sp.mel_scale.fb), _hip.ptr(lo),
                      _hip.ptr(hi), n_fft, 256, sp.n_mels, 1e-7, 1.0, 0, _hip.ptr(part), _hip.ptr(scratch), _hip.ptr(value),
                      dx.data_ptr(), dx.stride(0), _hip.stream())
        torch.cuda.synchronize()
        assert float(value) == 123.0 and bool((dx == 7.0).all())          # nothing was launched


# ---- effect_loss_grad through the LSTM BPTT, and the TBPTT step -----------------------------------------------------------
MIX = {"log_mel_l1": 0.5, "l1": 0.5, "mrstft": 0.3}


@pytest.mark.parametrize("weights,T", [({"log_mel_l1": 1.0}, 1024), ({"log_mel_l1": 1.0}, 4096), (MIX, 1500), (MIX, 4096)])
def test_lstm_bptt_log_mel_loss_vs_autograd(dev, weights, T):
    """mx_lstm_bwd with d loss / d y from effect_loss_grad (log_mel_l1 alone and beside l1 + mrstft) against torch autograd
    through nn.LSTM and the oracle's loss modules; the 2e-3 gate of the mrstft cases (fp32 gradients divided by band
    levels on both sides).  The mix runs at 1500 samples instead of 1024: the MR-STFT's 2048-point resolution needs more than
    1024 (torch.stft's reflect padding refuses such a chunk in the oracle as well)."""
    from mod_extraction_amd import effect_losses, models as am
    from oracle import losses as olosses, models as om
    torch.manual_seed(13)
    x = torch.rand(B, 1, 1024 + T) * 1.6 - 0.8
    lat = torch.rand(B, 1, 1024 + T)
    wet = (0.6 * x + 0.3 * torch.roll(x, 2, -1)).clamp(-1, 1)
    sd = om.LSTMEffectModel(1, 1, 64, 1).state_dict()
    ref = om.LSTMEffectModel(1, 1, 64, 1); ref.load_state_dict(sd)
    mine = am.LSTMEffectModel(1, 1, 64, 1); mine.load_state_dict(sd); mine = mine.to(dev)
    ref.clear_hidden(); ref(x[..., :1024], lat[..., :1024]); ref.detach_hidden()
    y_r = ref(x[..., 1024:], lat[..., 1024:])
    y_r.retain_grad()
    loss_r = sum(w * olosses.get_loss_func_by_name(k)(y_r, wet[..., 1024:]) for k, w in weights.items())
    loss_r.backward()
    xd, ld, wd = x.to(dev), lat.to(dev), wet.to(dev)
    mine.clear_hidden(); mine.run_chunk(xd[..., :1024], ld[..., :1024]); mine.detach_hidden()
    stash = torch.empty((B, T, 384), device=dev)
    y_m, h0, c0 = mine.run_chunk(xd[..., 1024:], ld[..., 1024:], stash)
    dy = effect_losses.effect_loss_grad(y_m, wd[..., 1024:].contiguous(), weights)
    e_dy = float((dy.cpu() - y_r.grad[:, 0]).abs().max() / y_r.grad.abs().max())
    grad = torch.empty(am.LSTM_NPARAM, device=dev)
    mine.bptt_chunk(xd[..., 1024:], ld[..., 1024:], y_m, dy, stash, h0, c0, grad)
    off, worst = 0, 0.0
    for n, p in ref.named_parameters():
        k = p.numel()
        a, r = grad[off:off + k].cpu(), p.grad.reshape(-1)
        e = float((a - r).abs().max() / r.abs().max())
        worst = max(worst, e)
        assert e < 2e-3, (n, e)
        off += k
    assert off == am.LSTM_NPARAM
    print(f"[measured] d loss / d y ({'+'.join(weights)}, T={T}): rel err {e_dy:.2e}; LSTM parameters {worst:.2e}")
    assert e_dy < 2e-3, e_dy


@pytest.mark.parametrize("ld,S,n", [({"log_mel_l1": 1.0, "l1": 0.5}, 1024, 6000), ({"log_mel_l1": 1.0}, 4096, 14000)])
@pytest.mark.parametrize("n_hidden", [64, 32])
def test_tbptt_training_with_log_mel_loss_vs_oracle(dev, ld, S, n, n_hidden):
    """TBPTTLFOEffectModeling with log_mel_l1 weighted (the constructor refused it before): optimizer steps, wet_hat, the
    loss, the logged terms and the weights after the steps against the oracle running torch autograd + torch.optim.AdamW.
    n_hidden 64: the fused LSTM-64 kernels (mx_lstm_bwd); 32: the general path (_general_train_chunk, autograd node)."""
    from mod_extraction_amd import lightning as al, models as am, optim
    from oracle import lightning as ol, models as om, modulations as omod
    W = 1024
    torch.manual_seed(W + S + n_hidden)
    dry = torch.rand(B, 1, n) * 1.6 - 0.8
    wet = (0.7 * dry + 0.2 * torch.roll(dry, 5, -1)).clamp(-1, 1)
    lfo = torch.stack([omod.make_mod_signal(64, 64 / (n / 44100.0), f, p, "cos") for f, p in ((6.0, 0.2), (9.0, 1.0), (7.5, 3.0))])
    ref = om.LSTMEffectModel(1, 1, n_hidden, 1)
    init = {k: v.clone() for k, v in ref.state_dict().items()}
    em = am.LSTMEffectModel(1, 1, n_hidden, 1); em.load_state_dict(init)
    assert bool(getattr(em, "generic", False)) == (n_hidden != 64)
    mod = al.TBPTTLFOEffectModeling(W, S, em, lfo_model=None, model_smooth_n_frames=0, should_stretch=False,
                                    discard_invalid_lfos=False, loss_dict=ld).to(dev).train()
    opt = optim.FlatAdamW(mod.parameters(), lr=1e-3, betas=(0.8, 0.99))
    loss, dd, _ = mod.common_step((dry.to(dev), wet.to(dev), lfo.to(dev), None), is_training=True, optimizer=opt, world_size=1)
    ropt = torch.optim.AdamW(ref.parameters(), lr=1e-3, betas=(0.8, 0.99))
    res = ol.tbptt_common_step(ref, ropt, dry, wet, lfo, W, S, ld, is_training=True, model_smooth_n_frames=0,
                               should_stretch=False, discard_invalid_lfos=False)
    assert opt.step_count == res["steps"] == (n - W) // S
    e_wet = float((dd["wet_hat"].cpu() - res["wet_hat"]).abs().max())
    e_loss = abs(float(loss) - float(res["loss"])) / max(1.0, abs(float(res["loss"])))
    print(f"[measured] TBPTT {ld} (n_hidden={n_hidden}): wet_hat {e_wet:.1e}, loss {e_loss:.1e}")
    assert e_wet < 1e-4
    assert e_loss < 1e-5
    for k in ld:
        assert abs(float(mod.logged[f"train/{k}"][-1]) - float(res["terms"][k])) < 1e-5 * max(1.0, abs(float(res["terms"][k]))), k
    for k, v in em.state_dict().items():
        d = (v.cpu() - ref.state_dict()[k]).abs()
        moved = (ref.state_dict()[k] - init[k]).abs()
        assert float(d.median()) < 0.02 * max(float(moved.median()), 1e-9), k
    assert mod._extra_losses["log_mel_l1"] is mod._grad_modules()["logmel"]         # one module: gradient and logging

"""CPU: the surface of the pre-emphasised ESR -- the three new C-ABI entries beside the header, their argument checks
(made before any launch, so they run without a device), "esr_pre" in GRAD_NAMES and the loss factory, the constructor
validation of the two audio-loss steps, and the object graph of configs/train_em_dry_wet_pre_emph.yml."""
import ctypes
import os

import pytest
import torch

from tests.test_abi import header_arg_counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mx_pre_emph", "mx_pre_emph_esr_sums", "mx_pre_emph_esr_grad")


@pytest.fixture(scope="module")
def lib():
    from mod_extraction_amd import _hip, build
    build.build(verbose=False)
    return _hip.load()


def test_new_entry_points_are_declared_bound_and_exported(lib):
    from mod_extraction_amd import _hip
    counts = header_arg_counts()
    for name in NEW:
        assert name in counts and name in _hip.SIGNATURES
        assert len(_hip.SIGNATURES[name]) == counts[name], name
        assert hasattr(lib, name)
        assert set(_hip.SIGNATURES[name]) <= {ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float}
    assert _hip.ABI_VERSION == 21 and lib.mx_abi_version() == 21


def test_argument_checks_come_before_any_launch(lib):
    """Never dereferenced: the pointers below are arbitrary non-NULL values, every call must be refused by its checks."""
    p = 4096
    ARG, UNSUPPORTED = -1, -2
    # mx_pre_emph(x, x_stride, B, T, taps, K, low_pass, transpose, out, out_stride, stream)
    assert lib.mx_pre_emph(None, 8, 1, 8, p, 2, 0, 0, p, 8, None) == ARG
    assert lib.mx_pre_emph(p, 8, 1, 8, None, 2, 0, 0, p, 8, None) == ARG
    assert lib.mx_pre_emph(p, 8, 1, 8, p, 2, 0, 0, None, 8, None) == ARG
    assert lib.mx_pre_emph(p, 8, 0, 8, p, 2, 0, 0, p, 8, None) == ARG
    assert lib.mx_pre_emph(p, 8, 1, 0, p, 2, 0, 0, p, 8, None) == ARG
    assert lib.mx_pre_emph(p, 1, 1, 1, p, 2, 1, 0, p, 1, None) == ARG              # T == 1 with low_pass: L == 0
    assert lib.mx_pre_emph(p, 8, 1, 8, p, 2, 0, 0, p, 7, None) == ARG              # out_stride < L
    assert lib.mx_pre_emph(p, 8, 1, 8, p, 2, 1, 1, p, 7, None) == ARG              # transposed: out_stride < T
    assert lib.mx_pre_emph(p, 8, 1, 8, p, 0, 0, 0, p, 8, None) == UNSUPPORTED
    assert lib.mx_pre_emph(p, 8, 1, 8, p, 17, 0, 0, p, 8, None) == UNSUPPORTED
    # mx_pre_emph_esr_sums(y_hat, hs, y, ys, B, T, taps, K, low_pass, part, stream)
    assert lib.mx_pre_emph_esr_sums(p, 8, p, 8, 1, 8, p, 2, 0, None, None) == ARG
    assert lib.mx_pre_emph_esr_sums(p, 8, p, 8, 0, 8, p, 2, 0, p, None) == ARG
    assert lib.mx_pre_emph_esr_sums(p, 1, p, 1, 1, 1, p, 2, 1, p, None) == ARG
    assert lib.mx_pre_emph_esr_sums(p, 8, p, 8, 1, 8, p, 0, 0, p, None) == UNSUPPORTED
    assert lib.mx_pre_emph_esr_sums(p, 8, p, 8, 1, 8, p, 17, 0, p, None) == UNSUPPORTED
    # mx_pre_emph_esr_grad(y_hat, hs, y, ys, B, T, taps, K, low_pass, w, eps, accumulate, part, dy, dy_stride, stream)
    assert lib.mx_pre_emph_esr_grad(p, 8, p, 8, 1, 8, p, 2, 0, 1.0, 1e-8, 0, p, None, 8, None) == ARG
    assert lib.mx_pre_emph_esr_grad(p, 8, p, 8, 1, 8, p, 2, 0, 1.0, 1e-8, 0, p, p, 7, None) == ARG       # dy_stride < T
    assert lib.mx_pre_emph_esr_grad(p, 8, p, 8, 1, 8, p, 2, 1, 1.0, 1e-8, 0, p, p, 7, None) == ARG       # ... also when L = T - 1
    assert lib.mx_pre_emph_esr_grad(p, 1, p, 1, 1, 1, p, 2, 1, 1.0, 1e-8, 0, p, p, 1, None) == ARG
    assert lib.mx_pre_emph_esr_grad(p, 8, p, 8, 1, 8, p, 17, 0, 1.0, 1e-8, 0, p, p, 8, None) == UNSUPPORTED
    assert lib.mx_pre_emph_esr_grad(p, 8, p, 8, 1, 8, p, 0, 0, 1.0, 1e-8, 0, p, p, 8, None) == UNSUPPORTED


def test_esr_pre_is_a_gradient_loss_and_a_factory_name():
    from mod_extraction_amd import effect_losses, losses, wright_code
    assert effect_losses.GRAD_NAMES[-1] == "esr_pre"
    assert effect_losses.GRAD_NAMES[:-1] == ("l1", "mse", "esr", "dc", "mrstft", "log_mel_l1")
    mod = losses.get_loss_func_by_name("esr_pre")
    assert isinstance(mod, losses.PreEmphESRLoss)
    assert mod.taps.filter_cfs == (-0.95, 1.0) and mod.taps.low_pass is False and mod.eps == 1e-8
    assert wright_code.WrightESRLoss().epsilon == 0.0 and wright_code.WrightDCLoss().epsilon == 0.0
    pe = wright_code.WrightPreEmph([-0.95, 1], low_pass=True)
    assert pe.zPad == 1 and pe.low_pass is True


def test_no_cpu_fallback_and_unknown_names_still_raise():
    from mod_extraction_amd import _hip, effect_losses, losses, wright_code
    x = torch.zeros(2, 1, 16)
    with pytest.raises(_hip.HipLibraryError):
        losses.PreEmphESRLoss()(x, x)
    with pytest.raises(_hip.HipLibraryError):
        wright_code.WrightPreEmph([-0.95, 1.0])(torch.zeros(16, 2, 1), torch.zeros(16, 2, 1))
    with pytest.raises(_hip.HipLibraryError):
        wright_code.WrightESRLoss()(torch.zeros(16, 2, 1), torch.zeros(16, 2, 1))
    with pytest.raises(NotImplementedError):
        effect_losses.effect_loss_grad(x, x, {"esr_pre": 1.0, "esr_post": 1.0})
    with pytest.raises(NotImplementedError):
        losses.PreEmphESRLoss()(x.clone().requires_grad_(True), x)                # forward-only under autograd


@pytest.mark.parametrize("cfs", [[], [0.1] * 17])
def test_steps_validate_the_taps_at_construction(cfs):
    from mod_extraction_amd import lightning, models
    with pytest.raises(ValueError):
        lightning.TBPTTLFOEffectModeling(1024, 1024, models.LSTMEffectModel(), loss_dict={"esr_pre": 1.0},
                                         pre_emph_filter_cfs=cfs)
    with pytest.raises(ValueError):
        lightning.LFOExtractionThroughEffect(torch.nn.Identity(), audio_loss_dict={"esr_pre": 1.0}, pre_emph_filter_cfs=cfs)


def test_steps_build_their_own_filter():
    from mod_extraction_amd import lightning, losses, models
    taps = [0.1 * i for i in range(1, 17)]
    a = lightning.TBPTTLFOEffectModeling(1024, 1024, models.LSTMEffectModel(), loss_dict={"esr_pre": 1.0, "dc": 1.0},
                                         pre_emph_filter_cfs=taps, pre_emph_low_pass=True)
    b = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), audio_loss_dict={"l1": 1.0, "esr_pre": 0.0},
                                             pre_emph_filter_cfs=taps, pre_emph_low_pass=True)
    for step in (a, b):
        mod = step._loss_module("esr_pre")
        assert isinstance(mod, losses.PreEmphESRLoss) and mod is step._loss_module("esr_pre")
        assert mod.taps.filter_cfs == tuple(float(c) for c in taps) and mod.taps.low_pass is True
        assert step._grad_modules()["pre_emph"] is mod
        assert "esr_pre" not in dict(step.named_modules())
    assert not a._fused_l1
    c = lightning.LFOExtractionThroughEffect(torch.nn.Identity(), audio_loss_dict={"l1": 1.0})
    assert c._grad_modules()["pre_emph"] is None and c._loss_module("esr_pre").taps.filter_cfs == (-0.95, 1.0)


def test_pre_emph_config_object_graph():
    from mod_extraction_amd import cli, lightning, models
    old = os.getcwd()
    os.chdir(os.path.join(ROOT, "scripts"))
    try:
        c = cli.CustomLightningCLI(args=["fit", "-c", "../configs/train_em_dry_wet_pre_emph.yml"], run=False,
                                   device=torch.device("cpu"), allow_missing_ckpt=True)
    finally:
        os.chdir(old)
    assert isinstance(c.model, lightning.TBPTTLFOEffectModeling) and isinstance(c.model.effect_model, models.LSTMEffectModel)
    assert c.model.loss_dict == {"l1": 0.0, "esr_pre": 1.0, "dc": 1.0} and not c.model._fused_l1
    assert c.model._loss_module("esr_pre").taps.filter_cfs == (-0.95, 1.0)
    assert c.model._loss_module("esr_pre").taps.low_pass is False
    assert sum(p.numel() for p in c.model.parameters() if p.requires_grad) == 17473
    # the same graph as train_em_dry_wet.yml but for the loss
    base = cli.load_config(os.path.join(ROOT, "configs", "train_em_dry_wet.yml"))
    mine = cli.load_config(os.path.join(ROOT, "configs", "train_em_dry_wet_pre_emph.yml"))
    for key in ("loss_dict", "pre_emph_filter_cfs", "pre_emph_low_pass"):
        base["model"]["init_args"].pop(key, None)
        mine["model"]["init_args"].pop(key, None)
    assert base == mine

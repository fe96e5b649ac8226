"""CPU: the surface of the LFO fit (K18) -- its declaration in include/modex_hip.h against ``_hip.SIGNATURES``, the limits of
``mx_lfo_fit`` (checked before any launch, so without a device), ``modulations.fit_lfo``'s errors, ``LFOFit``,
``LFOExtraction(fit_metrics=...)``'s construction, and a step without the argument.  No device work."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT_KEYS = ["val/fit_rate_err_hz", "val/fit_rate_err_rel", "val/fit_shape_acc", "val/fit_resid", "val/fit_label_resid"]


def test_header_table_and_symbol():
    """One entry point, declared in include/modex_hip.h (section K18) and bound from ``_hip.SIGNATURES``, which is derived
    from that text."""
    from mod_extraction_amd import _hip, build
    from tests.test_abi import header_arg_counts
    lib = ctypes.CDLL(build.build(verbose=False))
    counts = header_arg_counts()
    assert [n for n in counts if n.startswith("mx_lfo_fit")] == ["mx_lfo_fit"]
    assert hasattr(lib, "mx_lfo_fit") and counts["mx_lfo_fit"] == 19 == len(_hip.SIGNATURES["mx_lfo_fit"])
    assert _hip.ABI_VERSION == 21 == lib.mx_abi_version()
    assert _hip.load().mx_lfo_fit.argtypes == _hip.SIGNATURES["mx_lfo_fit"]           # load() binds the table
    zeros = {ctypes.c_void_p: None, ctypes.c_int64: 0, ctypes.c_int32: 0, ctypes.c_float: 0.0}
    assert _hip.load().mx_lfo_fit(*[zeros[t] for t in _hip.SIGNATURES["mx_lfo_fit"]]) == -1


def fit(B=4, n=345, sr=172.5, f_min=0.25, f_max=8.0, mask=0x3F, rate_div=4, J=32, L=4, y=8, stride=None, out=8, table=None):
    """``mx_lfo_fit`` on pointers that are never read: every case below is refused before a launch."""
    from mod_extraction_amd import _hip
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    outs = [p(out)] * 6 if not isinstance(out, (list, tuple)) else [p(v) for v in out]
    return _hip.load().mx_lfo_fit(p(y), n if stride is None else stride, B, n, sr, f_min, f_max, mask, rate_div, J, L, *outs,
                                  p(table), None)


def test_limits_are_checked_before_any_launch():
    ARG, UNSUPPORTED = -1, -2
    assert fit(y=None) == ARG and fit(B=0) == ARG and fit(B=-3) == ARG
    for k in range(6):                                                       # every output vector is required
        assert fit(out=[None if i == k else 8 for i in range(6)]) == ARG, k
    assert fit(f_min=0.0) == ARG and fit(f_min=-1.0) == ARG and fit(f_min=3.0, f_max=2.0) == ARG
    assert fit(f_max=86.25) == ARG and fit(f_max=100.0) == ARG and fit(f_min=float("nan")) == ARG
    assert fit(mask=0) == ARG and fit(mask=0x80) == ARG and fit(L=-1) == ARG and fit(stride=344) == ARG
    assert fit(n=15) == UNSUPPORTED and fit(n=4097, f_max=0.3) == UNSUPPORTED and fit(n=0) == UNSUPPORTED
    assert fit(J=3) == UNSUPPORTED and fit(J=129) == UNSUPPORTED and fit(L=9) == UNSUPPORTED
    assert fit(rate_div=0) == UNSUPPORTED and fit(rate_div=17) == UNSUPPORTED
    # K = floor((f_max - f_min) / df) + 1 with df = sr / (rate_div n): 345 points at 172.5 Hz and rate_div 16 have df = 1 / 32,
    # so 0.25 .. 16.21875 Hz is K = 512 (would launch: not tried here) and one df more is K = 513
    assert fit(f_max=16.25, rate_div=16) == UNSUPPORTED and fit(n=4096, sr=172.5, f_max=8.0) == UNSUPPORTED


def test_fit_lfo_errors_are_raised_before_the_launch(monkeypatch):
    from mod_extraction_amd import _hip, modulations as M
    calls = []
    monkeypatch.setattr(_hip, "call", lambda name, *a: calls.append(name))
    y = torch.zeros(3, 48)
    with pytest.raises(ValueError, match="unknown LFO shape"):
        M.fit_lfo(y, 24.0, (0.25, 4.0), shapes=["cos", "sine"])
    for shapes in ([], (), "cos"):
        with pytest.raises(ValueError, match="non-empty"):
            M.fit_lfo(y, 24.0, (0.25, 4.0), shapes=shapes)
    for window in ((0.0, 4.0), (-1.0, 4.0), (3.0, 2.0), (0.25, 12.0), (0.25, 13.0), (1.0,), 2.0, (1.0, 2.0, 3.0), ("a", "b")):
        with pytest.raises(ValueError, match="rate_hz"):
            M.fit_lfo(y, 24.0, window)
    with pytest.raises(ValueError, match="HIP device"):
        M.fit_lfo(y, 24.0, (0.25, 4.0))                                       # a CPU tensor: there is no fallback
    with pytest.raises(ValueError, match="fp32"):
        M.fit_lfo(y.double(), 24.0, (0.25, 4.0))
    with pytest.raises(ValueError, match="fp32"):
        M.fit_lfo(torch.zeros(2, 3, 48), 24.0, (0.25, 4.0))
    assert calls == []
    assert M.LFO_SHAPES == ("cos", "rect_cos", "inv_rect_cos", "tri", "saw", "rsaw") and M.fit_shape_mask(M.LFO_SHAPES) == 0x3F
    assert M.fit_shape_mask(["sqr", "cos"]) == 0x41 and M.SHAPE_NAMES[6] == "sqr"


def test_lfofit_is_a_named_tuple():
    from mod_extraction_amd import modulations as M
    v = [torch.tensor([4, 0, 6], dtype=torch.int32)] + [torch.zeros(3) for _ in range(5)]
    f = M.LFOFit(*v)
    assert f._fields == ("shape", "rate_hz", "phase", "amp", "offset", "resid", "per_shape_resid") and f.per_shape_resid is None
    assert f.shape_names() == ["saw", "cos", "sqr"] and f.rate_hz is v[1] and tuple(f)[:6] == tuple(v)


class Stub(torch.nn.Module):
    """A model that returns the (lfo, latent) pair it was built with."""

    def __init__(self, out):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.out = out

    def forward(self, x):
        return self.out, None


def test_fit_metrics_are_checked_at_construction():
    from mod_extraction_amd import lightning, trainer
    mk = lambda **kw: lightning.LFOExtraction(torch.nn.Linear(3, 2), **kw)
    step = mk(fit_metrics={"rate_hz": [0.25, 8.0]})
    assert step.fit_metrics == {"rate_hz": (0.25, 8.0), "shapes": ["cos", "rect_cos", "inv_rect_cos", "tri", "saw", "rsaw"]}
    assert trainer.metric_names(step, "val") == ["val/l1", "val/mse", "val/loss"] + FIT_KEYS
    assert trainer.metric_names(step, "train") == ["train/l1", "train/mse", "train/loss"]
    full = mk(fit_metrics={"rate_hz": (0.5, 3.0), "shapes": ["tri", "sqr"], "rate_div": 8, "n_phases": 64, "n_rounds": 2})
    assert full.fit_metrics == {"rate_hz": (0.5, 3.0), "shapes": ["tri", "sqr"], "rate_div": 8, "n_phases": 64, "n_rounds": 2}
    plain = mk()
    assert plain.fit_metrics is None and trainer.metric_names(plain, "val") == ["val/l1", "val/mse", "val/loss"]
    assert list(step.state_dict()) == list(plain.state_dict())
    for bad in ({}, {"shapes": ["cos"]}, [0.25, 8.0], {"rate_hz": [0.25]}, {"rate_hz": [0.0, 8.0]}, {"rate_hz": [3.0, 2.0]},
                {"rate_hz": [0.25, 8.0], "shapes": []}, {"rate_hz": [0.25, 8.0], "shapes": ["sine"]},
                {"rate_hz": [0.25, 8.0], "rate": 4}, {"rate_hz": [0.25, 8.0], "rate_div": 0}, {"rate_hz": [0.25, 8.0], "n_phases": 3},
                {"rate_hz": [0.25, 8.0], "n_rounds": 9}, {"rate_hz": [0.25, 8.0], "n_rounds": 1.5}):
        with pytest.raises(ValueError):
            mk(fit_metrics=bad)


def test_steps_without_the_argument_and_training_steps_do_not_fit(monkeypatch):
    """The LFO losses are HIP: a torch stand-in lets the step run here.  Without ``fit_metrics`` a validation step logs exactly
    the loss names and ``data_dict`` has the parent's keys; with it, a TRAINING step is the same (no fit), and a validation
    step reaches ``fit_lfo``, which refuses the CPU tensor (no fallback)."""
    from mod_extraction_amd import lightning

    def lfo_loss(y_hat, y, weights):
        terms = {k: (y_hat - y).abs().mean() for k in weights}
        return sum(w * terms[k] for k, w in weights.items()), terms

    monkeypatch.setattr(lightning.L, "lfo_loss", lfo_loss)
    fitted = []
    real = lightning.fit_lfo
    monkeypatch.setattr(lightning, "fit_lfo", lambda *a, **kw: fitted.append(kw) or real(*a, **kw))
    lfo = torch.rand(4, 1, 48)
    batch = (torch.zeros(4, 1, 512), torch.zeros(4, 1, 512), lfo[:, 0].clone(), None)
    keys = ["dry", "mod_sig", "mod_sig_hat", "wet"]
    plain = lightning.LFOExtraction(Stub(lfo), sr=256.0, model_smooth_n_frames=1)
    _, data, _ = plain.validation_step(batch)
    assert sorted(plain.logged) == ["val/l1", "val/loss", "val/mse"] and sorted(data) == keys
    plain.logged.clear()
    plain.training_step(batch)
    assert sorted(plain.logged) == ["train/l1", "train/loss", "train/mse"]
    step = lightning.LFOExtraction(Stub(lfo), sr=256.0, model_smooth_n_frames=1, fit_metrics={"rate_hz": [0.25, 4.0]})
    step.training_step(batch)
    assert sorted(step.logged) == ["train/l1", "train/loss", "train/mse"] and fitted == []
    with pytest.raises(ValueError, match="HIP device"):
        step.validation_step(batch)
    assert len(fitted) == 1 and fitted[0]["rate_hz"] == (0.25, 4.0)


def test_shipped_config():
    from mod_extraction_amd import cli, lightning
    old = os.getcwd()
    os.chdir(os.path.join(ROOT, "scripts"))
    try:
        mk = lambda name: cli.CustomLightningCLI(args=["validate", "-c", f"../configs/{name}"], run=False,
                                                 device=torch.device("cpu"), allow_missing_ckpt=True)
        c, base = mk("eval_lfo_fit.yml"), mk("eval_lfo.yml")
    finally:
        os.chdir(old)
    assert isinstance(c.model, lightning.LFOExtraction) and c.model.fit_metrics["rate_hz"] == (0.25, 8.0)
    assert base.model.fit_metrics is None
    strip = lambda cfg: {k: v for k, v in cfg["model"]["init_args"].items() if k != "fit_metrics"}
    assert strip(c.config) == strip(base.config) and c.config["data"] == base.config["data"]

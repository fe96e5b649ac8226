"""CPU: the trainer keys `gradient_clip_val`, `gradient_clip_algorithm` and `accumulate_grad_batches` are validated, travel from
the YAML `trainer:` section into `trainer.Trainer` and on to the optimizer, and the accumulation window drives the optimizer in
the documented order (no kernels run here: stub module, recording stub optimizer)."""
import contextlib
import json
import os

import pytest
import torch

from mod_extraction_amd import cli, lightning, optim, trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def _params():
    return [torch.nn.Parameter(torch.zeros(5, 3)), torch.nn.Parameter(torch.zeros(7))]


# ---- argument checking ------------------------------------------------------------------------------------------------
def test_trainer_defaults_and_nulls():
    for kw in ({}, dict(gradient_clip_val=None, gradient_clip_algorithm=None, accumulate_grad_batches=None)):
        t = trainer.Trainer(log_fn=None, **kw)
        assert t.gradient_clip_val is None and t.gradient_clip_algorithm == "norm" and t.accumulate_grad_batches == 1
    t = trainer.Trainer(log_fn=None, gradient_clip_val=0.5, gradient_clip_algorithm="value", accumulate_grad_batches=4)
    assert (t.gradient_clip_val, t.gradient_clip_algorithm, t.accumulate_grad_batches) == (0.5, "value", 4)
    assert trainer.Trainer(log_fn=None, gradient_clip_val=0).gradient_clip_val is None          # Lightning: <= 0 is off
    assert trainer.Trainer(log_fn=None, gradient_clip_val=-1.0).gradient_clip_val is None
    assert trainer.Trainer(log_fn=None, gradient_clip_val=2).gradient_clip_val == 2.0


@pytest.mark.parametrize("kw", [dict(gradient_clip_algorithm="l2"), dict(gradient_clip_val=1.0, gradient_clip_algorithm="inf"),
                                dict(gradient_clip_val="1.0"), dict(gradient_clip_val=float("nan")),
                                dict(gradient_clip_val=float("inf")), dict(gradient_clip_val=True),
                                dict(accumulate_grad_batches=0), dict(accumulate_grad_batches=-2),
                                dict(accumulate_grad_batches=2.5), dict(accumulate_grad_batches=2.0),
                                dict(accumulate_grad_batches="2"), dict(accumulate_grad_batches=True)])
def test_trainer_refuses_bad_values(kw):
    with pytest.raises(ValueError):
        trainer.Trainer(log_fn=None, **kw)


def test_flat_adamw_clip_arguments():
    o = optim.FlatAdamW(_params())
    assert o.clip_val is None and o.clip_algorithm == "norm" and o.last_grad_norm is None and o.last_clip_scale is None
    o = optim.FlatAdamW(_params(), clip_val=0.25, clip_algorithm="value")
    assert (o.clip_val, o.clip_algorithm) == (0.25, "value")
    o.set_gradient_clip(1.5, "norm")
    assert (o.clip_val, o.clip_algorithm) == (1.5, "norm")
    assert o._clip_stat.dtype == torch.float64 and o._clip_stat.numel() == 2
    assert o._clip_part.dtype == torch.float64 and o._clip_part.numel() == optim.sumsq_partials(o.numel) == 1
    stat = o._clip_stat
    for off in (None, 0, 0.0, -3.0):
        o.set_gradient_clip(off, "norm")
        assert o.clip_val is None
    o.set_gradient_clip(2.0, None)
    assert o.clip_val == 2.0 and o.clip_algorithm == "norm" and o._clip_stat is stat            # workspaces allocated once
    for bad in ("l1", "Norm", 2):
        with pytest.raises(ValueError):
            o.set_gradient_clip(1.0, bad)
        with pytest.raises(ValueError):
            optim.FlatAdamW(_params(), clip_val=1.0, clip_algorithm=bad)
    with pytest.raises(ValueError):
        optim.FlatAdamW(_params(), clip_val="big")


def test_clip_settings_travel_in_the_optimizer_state_dict():
    a = optim.FlatAdamW(_params(), clip_val=0.75, clip_algorithm="value")
    sd = a.state_dict()
    assert sd["clip_val"] == 0.75 and sd["clip_algorithm"] == "value"
    b = optim.FlatAdamW(_params())
    b.load_state_dict(sd)
    assert (b.clip_val, b.clip_algorithm) == (0.75, "value")
    old = {k: v for k, v in sd.items() if not k.startswith("clip_")}          # a state dict from before the clip existed
    c = optim.FlatAdamW(_params(), clip_val=3.0)
    c.load_state_dict(old)
    assert (c.clip_val, c.clip_algorithm) == (3.0, "norm")                     # read back only when present
    # the Lightning-layout checkpoint does not change
    assert set(trainer.adamw_state_dict(a)["param_groups"][0]) == set(trainer.adamw_state_dict(b)["param_groups"][0])
    assert "clip_val" not in trainer.adamw_state_dict(a)["param_groups"][0]


# ---- YAML -> Trainer -> optimizer ------------------------------------------------------------------------------------
def _write_config(tmp_path, trainer_section, opt_args=""):
    cfgs = os.path.join(ROOT, "configs")
    opt = tmp_path / "opt.yml"
    opt.write_text("class_path: torch.optim.AdamW\ninit_args:\n  lr: 1e-4\n  betas: [0.8, 0.99]\n" + opt_args)
    path = tmp_path / "train.yml"
    path.write_text(f"""seed_everything: 43
trainer: {trainer_section}
data: {cfgs}/data/interwoven_synth.yml
model:
  class_path: mod_extraction.lightning.LFOExtraction
  init_args:
    model: {cfgs}/models/spectral_2dcnn.yml
    use_dry: true
    model_smooth_n_frames: 0
    should_stretch: false
    loss_dict: {{l1: 1.0, fdl1: 5.0, sdl1: 10.0, mse: 0.0}}
optimizer: {opt}
""")
    return str(path)


class _NoData:
    def train_steps_per_epoch(self):
        return 0

    def val_steps_per_epoch(self):
        return 0


def test_cli_forwards_the_three_keys_to_trainer_and_optimizer(tmp_path):
    path = _write_config(tmp_path, "{max_epochs: 1, num_sanity_val_steps: 0, gradient_clip_val: 0.5, "
                                   "gradient_clip_algorithm: value, accumulate_grad_batches: 3}")
    c = cli.CustomLightningCLI(args=["fit", "-c", path], run=False, device=CPU)
    t = c.trainer
    assert (t.gradient_clip_val, t.gradient_clip_algorithm, t.accumulate_grad_batches) == (0.5, "value", 3)
    opt = cli.instantiate(c.optimizer_spec, params=[p for p in c.model.parameters() if p.requires_grad])
    assert isinstance(opt, optim.FlatAdamW) and opt.clip_val is None
    t.fit(c.model, _NoData(), opt)                              # fit's set-up puts the trainer's clip on the optimizer
    assert (opt.clip_val, opt.clip_algorithm) == (0.5, "value")
    assert opt.step_count == 0


def test_cli_null_keys_are_the_defaults_and_optimizer_init_args_reach_the_clip(tmp_path):
    path = _write_config(tmp_path, "{max_epochs: 1, num_sanity_val_steps: 0, gradient_clip_val: null, "
                                   "gradient_clip_algorithm: null, accumulate_grad_batches: null}",
                         opt_args="  clip_val: 2.0\n  clip_algorithm: norm\n")
    c = cli.CustomLightningCLI(args=["fit", "-c", path], run=False, device=CPU)
    t = c.trainer
    assert (t.gradient_clip_val, t.gradient_clip_algorithm, t.accumulate_grad_batches) == (None, "norm", 1)
    opt = cli.instantiate(c.optimizer_spec, params=[p for p in c.model.parameters() if p.requires_grad])
    assert (opt.clip_val, opt.clip_algorithm) == (2.0, "norm")
    t.fit(c.model, _NoData(), opt)                              # no trainer-level clip: the optimizer's own setting stands
    assert (opt.clip_val, opt.clip_algorithm) == (2.0, "norm")


def test_cli_refuses_a_bad_key_in_the_yaml(tmp_path):
    path = _write_config(tmp_path, "{max_epochs: 1, accumulate_grad_batches: 0}")
    with pytest.raises(ValueError):
        cli.CustomLightningCLI(args=["fit", "-c", path], run=False, device=CPU)


def test_a_trained_config_of_the_reference_still_builds_with_the_three_keys_at_their_defaults(tmp_path, golden_dir):
    """configs/trained/*.yml of the reference carry the three keys as `null` (kept as data in
    tests/golden/reference_configs.json; written back out in the reference's layout so that its indirections resolve)."""
    import yaml
    with open(os.path.join(golden_dir, "reference_configs.json")) as f:
        entries = json.load(f)
    for rel, cfg in entries.items():
        p = tmp_path / "configs" / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(yaml.safe_dump(cfg, sort_keys=False))
    rel = next(r for r in sorted(entries) if r.startswith("trained/lfo_2dcnn_io_sa_25_25__ph_fl_ch_all_2__idmt_4__"))
    section = entries[rel]["trainer"]
    assert {"gradient_clip_val", "gradient_clip_algorithm", "accumulate_grad_batches"} <= set(section)
    assert section["gradient_clip_val"] is None and section["accumulate_grad_batches"] is None
    old = os.getcwd()
    os.chdir(tmp_path / "configs")
    try:
        c = cli.CustomLightningCLI(args=["fit", "-c", str(tmp_path / "configs" / rel)], run=False, device=CPU,
                                   allow_missing_ckpt=True)
    finally:
        os.chdir(old)
    assert isinstance(c.model, lightning.LFOExtraction)
    t = c.trainer
    assert (t.gradient_clip_val, t.gradient_clip_algorithm, t.accumulate_grad_batches) == (None, "norm", 1)


# ---- manual optimization ---------------------------------------------------------------------------------------------
class _Manual:
    automatic_optimization = False


@pytest.mark.parametrize("kw", [dict(gradient_clip_val=1.0), dict(gradient_clip_val=1.0, gradient_clip_algorithm="value"),
                                dict(accumulate_grad_batches=2)])
def test_fit_refuses_trainer_level_clip_and_accumulation_for_a_manual_module(kw):
    with pytest.raises(ValueError, match="clip_val"):
        trainer.Trainer(log_fn=None, **kw).fit(_Manual(), _NoData(), optim.FlatAdamW(_params()))


# ---- the accumulation schedule ---------------------------------------------------------------------------------------
class _Loss:
    def __init__(self, log, i, opt):
        self.log, self.i, self.opt = log, i, opt

    def backward(self):
        self.log.append(("backward", self.i, "direct" if self.opt.in_direct else "plain"))


class _Module:
    loss_dict = {}

    def __init__(self, log, opt, none_at):
        self.log, self.opt, self.none_at, self.logged = log, opt, set(none_at), {}

    def train(self):
        return self

    def eval(self):
        return self

    def training_step(self, batch, idx):
        return None if batch in self.none_at else _Loss(self.log, batch, self.opt)


class _Optimizer:
    def __init__(self, log):
        self.log, self.in_direct, self.step_count = log, False, 0
        self.flat_grad = torch.zeros(4)

    def zero_grad(self):
        self.log.append(("zero_grad",))

    @contextlib.contextmanager
    def direct_backward(self):
        self.in_direct = True
        try:
            yield
        finally:
            self.in_direct = False

    def step(self, grad_scale=1.0):
        self.step_count += 1
        self.log.append(("step", grad_scale))

    def set_gradient_clip(self, val, algorithm):
        self.log.append(("clip", val, algorithm))


class _Data:
    def __init__(self, n):
        self.n, self.i = n, 0

    def train_steps_per_epoch(self):
        return self.n

    def val_steps_per_epoch(self):
        return 0

    def train_batch(self):
        self.i += 1
        return self.i - 1


def _run_schedule(monkeypatch, k, n, none_at, world_scale=1.0, **kw):
    log = []
    monkeypatch.setattr(trainer, "allreduce_flat_grad", lambda g, w: (log.append(("allreduce",)), world_scale)[1])
    opt = _Optimizer(log)
    t = trainer.Trainer(max_epochs=1, log_fn=None, accumulate_grad_batches=k, **kw)
    assert t.env["world_size"] == 1
    t.fit(_Module(log, opt, none_at), _Data(n), opt)
    return log, opt


def test_accumulation_schedule_k3_over_7_batches_with_one_none(monkeypatch):
    log, opt = _run_schedule(monkeypatch, 3, 7, none_at=[4], world_scale=0.5, gradient_clip_val=0.25)
    s = 0.5 / 3                                                  # scale / k, also for the short last window
    assert log == [
        ("clip", 0.25, "norm"),
        ("zero_grad",), ("backward", 0, "direct"),
        ("backward", 1, "plain"),
        ("backward", 2, "plain"), ("allreduce",), ("step", s),
        ("zero_grad",), ("backward", 3, "direct"),
        # batch 4 returned None: it contributes nothing
        ("backward", 5, "plain"), ("allreduce",), ("step", s),
        ("zero_grad",), ("backward", 6, "direct"), ("allreduce",), ("step", s),
    ]
    assert opt.step_count == 3


def test_accumulation_window_whose_first_batch_is_none_and_window_without_any_backward(monkeypatch):
    log, opt = _run_schedule(monkeypatch, 2, 5, none_at=[0, 2, 3])
    assert log == [
        ("zero_grad",),                                          # batch 0: None, the window still opens
        ("backward", 1, "plain"), ("allreduce",), ("step", 0.5),
        ("zero_grad",),                                          # batches 2 and 3: no backward in the window -> no step
        ("zero_grad",), ("backward", 4, "direct"), ("allreduce",), ("step", 0.5),
    ]
    assert opt.step_count == 2


def test_k1_is_the_parents_schedule_and_the_old_signature_still_works(monkeypatch):
    log, opt = _run_schedule(monkeypatch, 1, 3, none_at=[1])
    assert log == [("zero_grad",), ("backward", 0, "direct"), ("allreduce",), ("step", 1.0),
                   ("zero_grad",),
                   ("zero_grad",), ("backward", 2, "direct"), ("allreduce",), ("step", 1.0)]
    del log[:]
    t = trainer.Trainer(log_fn=None)
    loss = t.train_step(_Module(log, opt, []), opt, 9)          # train_step(module, optimizer, batch): one-batch window
    assert isinstance(loss, _Loss)
    assert log == [("zero_grad",), ("backward", 9, "direct"), ("allreduce",), ("step", 1.0)]
    assert t.train_step(_Module(log, opt, [9]), opt, 9) is None

"""Host mirror of mod_extraction/lightning.py: the step logic of ``LFOExtraction``
(lightning.py:65-199) and ``TBPTTLFOEffectModeling`` (lightning.py:202-431) with the same
constructor arguments, batch 4-tuple ``(dry, wet, mod_sig, fx_params)`` and metric names
(``train/l1`` ... ``val/loss``).  ``pytorch_lightning`` is replaced by ``trainer.Trainer`` (a thin
DDP loop); these classes are plain ``nn.Module``s that record their metrics in ``self.logged``.

Everything stays on the device: the reference's per-step ``.detach().float().cpu()`` copies of all
tensors (lightning.py:132-141) are dropped -- ``data_dict`` holds device tensors.
"""
import logging
import os
from collections import defaultdict
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor as T, nn

from . import losses as L
from .models import HiddenStateModel, RandomLFO
from .modulations import (LFO_SHAPES, LFOFit, find_valid_mod_sig_indices, fit_lfo, fit_rate_window, fit_shape_mask, smoothen, smoothen_bwd,
                          smoothen_with_grad, stretch_corners, stretch_corners_bwd, valid_mod_sig_mask)
from .util import linear_interpolate_last_dim, linear_interpolate_last_dim_bwd

log = logging.getLogger(__name__)
log.setLevel(level=os.environ.get("LOGLEVEL", "INFO"))


def stack_dry_wet(dry: T, wet: T) -> T:
    """``tr.cat([dry, wet], dim=1)`` (lightning.py:109,256).  The device batcher renders dry and wet as the two channels of
    ONE (B, 2, N) buffer: then the concatenation already exists and a view of it is returned (no 180 MB copy per step)."""
    B, C, N = dry.shape
    if (C == 1 and wet.shape == dry.shape and dry.dtype == wet.dtype and dry.stride() == wet.stride() == (2 * N, N, 1)
            and wet.data_ptr() == dry.data_ptr() + N * dry.element_size()
            and dry.untyped_storage().data_ptr() == wet.untyped_storage().data_ptr()):
        return torch.as_strided(dry, (B, 2, N), (2 * N, N, 1))
    return torch.cat([dry, wet], dim=1)


class BaseLightingModule(nn.Module):
    default_loss_dict = {"l1": 1.0, "mse": 0.0}

    def __init__(self, loss_dict: Optional[Dict[str, float]] = None) -> None:
        super().__init__()
        if loss_dict is None:
            loss_dict = self.default_loss_dict
        self.loss_dict = dict(loss_dict)
        self._fused_lfo = all(k in ("l1", "fdl1", "sdl1", "mse") for k in self.loss_dict)
        self.loss_funcs = nn.ModuleList([] if self._fused_lfo else
                                        [L.get_loss_func_by_name(name) for name in self.loss_dict])
        self.logged: Dict[str, List[T]] = defaultdict(list)
        self._extra_losses = {}           # loss modules outside effect_loss_terms (mrstft, ...), built once, by name

    def log(self, name: str, value: T) -> None:
        """Stands in for LightningModule.log(on_epoch=True, sync_dist=True): values are kept as
        device scalars; the trainer reduces them to epoch means (and all-reduces across ranks)."""
        self.logged[name].append(value.detach())

    @staticmethod
    def weighted_sum(terms: Dict[str, T], weights: Dict[str, float]) -> Optional[T]:
        """sum_k w_k terms[k] over the positive weights, in the order of ``weights`` (the first term starts the sum); None
        without a positive weight."""
        loss = None
        for name, w in weights.items():
            if w > 0:
                loss = w * terms[name] if loss is None else loss + w * terms[name]
        return loss

    def calc_and_log_losses(self, y_hat: T, y: T, loss_dict: Dict[str, float], prefix: str, log_total: bool = True) -> Optional[T]:
        """lightning.py:33-62: weighted sum of the losses ``loss_dict`` names (those the constructor was given); zero-weight
        terms are only logged.  Every term is logged as ``{prefix}{name}``, the sum (``log_total``) as ``{prefix}loss``."""
        if self._fused_lfo:
            loss, terms = L.lfo_loss(y_hat, y, loss_dict)
        else:
            terms = {name: f(y_hat, y) for name, f in zip(loss_dict, self.loss_funcs)}
            loss = self.weighted_sum(terms, loss_dict)
        for name in loss_dict:
            self.log(f"{prefix}{name}", terms[name])
        if log_total:
            self.log(f"{prefix}loss", loss)
        return loss

    @staticmethod
    def center_crop_mod_sig(mod_sig: T, size: int) -> T:
        if size == mod_sig.size(-1):
            return mod_sig
        assert size < mod_sig.size(-1)
        padding = mod_sig.size(-1) - size
        pad_l = padding // 2
        return mod_sig[..., pad_l:pad_l + size]

    def _loss_module(self, name: str):
        """One module per loss name for the lifetime of the step object (the MR-STFT module owns window / twiddle tables on
        the device: building it per batch re-uploaded them); the same object serves the gradient and the logging.  A plain
        dict: these modules are no submodules and stay out of the state dict."""
        mod = self._extra_losses.get(name)
        if mod is None:
            if name == "esr_pre":               # the step's own filter, not the defaults of get_loss_func_by_name
                mod = L.PreEmphESRLoss(self.pre_emph_filter_cfs, self.pre_emph_low_pass)
            else:
                mod = L.get_loss_func_by_name(name)
            self._extra_losses[name] = mod
        return mod

    pre_emph_filter_cfs: Tuple[float, ...] = (-0.95, 1.0)        # the filter of "esr_pre" (Wright & Valimaki's pre-emphasis)
    pre_emph_low_pass = False

    def _set_pre_emph(self, filter_cfs: Sequence[float], low_pass: bool) -> None:
        """The ``pre_emph_filter_cfs`` / ``pre_emph_low_pass`` arguments of the audio-loss steps: checked here, at
        construction (ValueError for no tap or more than the kernels' 16), used by ``_loss_module("esr_pre")``."""
        from .wright_code import PreEmphTaps
        taps = PreEmphTaps(filter_cfs, low_pass)
        self.pre_emph_filter_cfs, self.pre_emph_low_pass = taps.filter_cfs, taps.low_pass

    def _grad_modules(self):
        """The loss modules ``effect_loss_grad`` reuses, by the dict that names the step's audio losses."""
        names = getattr(self, "audio_loss_dict", self.loss_dict)
        return {"mrstft": self._loss_module("mrstft") if "mrstft" in names else None,
                "logmel": self._loss_module("log_mel_l1") if "log_mel_l1" in names else None,
                "pre_emph": self._loss_module("esr_pre") if "esr_pre" in names else None}


class LFOExtraction(BaseLightingModule):
    def __init__(self,
                 model: nn.Module,
                 sr: float = 44100,
                 use_dry: bool = True,
                 model_smooth_n_frames: int = 4,
                 should_stretch: bool = False,
                 max_n_corners: int = 16,
                 stretch_smooth_n_frames: int = 0,
                 sub_batch_size: Optional[int] = None,
                 loss_dict: Optional[Dict[str, float]] = None,
                 fit_metrics: Optional[Dict[str, object]] = None) -> None:
        """``fit_metrics`` (e.g. ``{rate_hz: [0.25, 8.0]}``, optionally ``shapes``, ``rate_div``, ``n_phases``, ``n_rounds``):
        validation steps also fit rate, phase and shape (``modulations.fit_lfo``) to the prediction and to the label, in one
        launch on the stacked 2 B rows, log ``val/fit_*`` (``FIT_METRIC_NAMES``) as device scalars and put the prediction's
        ``LFOFit`` into ``data_dict["lfo_fit"]``.  The prediction is compared with the FIT OF THE LABEL, not with
        ``fx_params``: phaser rows, quasi-periodic / combined labels and the crop under ``model_smooth_n_frames`` need no special
        case, and ``val/fit_label_resid`` shows when the label itself is no plain periodic LFO.  Training steps never fit;
        without the argument nothing changes."""
        super().__init__(loss_dict)
        self.model = model
        self.sr = sr
        self.use_dry = use_dry
        self.model_smooth_n_frames = model_smooth_n_frames
        self.should_stretch = should_stretch
        self.max_n_corners = max_n_corners
        self.stretch_smooth_n_frames = stretch_smooth_n_frames
        self.sub_batch_size = sub_batch_size
        self.fit_metrics = self._check_fit_metrics(fit_metrics)
        self.val_metric_names = [f"val/{k}" for k in self.FIT_METRIC_NAMES] if self.fit_metrics is not None else []

    FIT_METRIC_NAMES = ("fit_rate_err_hz", "fit_rate_err_rel", "fit_shape_acc", "fit_resid", "fit_label_resid")

    @staticmethod
    def _check_fit_metrics(spec) -> Optional[Dict[str, object]]:
        """The keyword arguments of ``fit_lfo`` a ``fit_metrics`` dict stands for, checked at construction (ValueError)."""
        if spec is None:
            return None
        if not isinstance(spec, dict) or "rate_hz" not in spec:
            raise ValueError(f"fit_metrics must be a dict with the key rate_hz: [min, max], got {spec!r}")
        unknown = sorted(set(spec) - {"rate_hz", "shapes", "rate_div", "n_phases", "n_rounds"})
        if unknown:
            raise ValueError(f"fit_metrics: unknown keys {unknown} (known: rate_hz, shapes, rate_div, n_phases, n_rounds)")
        kw: Dict[str, object] = {"rate_hz": fit_rate_window(spec["rate_hz"], float("inf")),
                                 "shapes": list(spec.get("shapes", LFO_SHAPES))}
        fit_shape_mask(kw["shapes"])
        for key, lo, hi in (("rate_div", 1, 16), ("n_phases", 4, 128), ("n_rounds", 0, 8)):
            if key in spec:
                v = spec[key]
                if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                    raise ValueError(f"fit_metrics: {key} must be an integer in [{lo}, {hi}], got {v!r}")
                kw[key] = v
        return kw

    def _fit_and_log(self, mod_sig_hat: T, mod_sig: T, lfo_sr: float):
        """One ``mx_lfo_fit`` launch on [prediction; label]; logs the five ``val/fit_*`` scalars (no host sync) and returns the
        prediction's ``LFOFit``."""
        bs = mod_sig_hat.size(0)
        both = fit_lfo(torch.cat([mod_sig_hat.detach().float(), mod_sig.detach().float()], dim=0), lfo_sr, **self.fit_metrics)
        hat, lab = LFOFit(*[v[:bs] for v in both[:6]]), LFOFit(*[v[bs:] for v in both[:6]])
        err = (hat.rate_hz - lab.rate_hz).abs()
        self.log("val/fit_rate_err_hz", err.mean())
        self.log("val/fit_rate_err_rel", (err / lab.rate_hz).mean())
        self.log("val/fit_shape_acc", (hat.shape == lab.shape).float().mean())
        self.log("val/fit_resid", hat.resid.mean())
        self.log("val/fit_label_resid", lab.resid.mean())
        return hat

    def common_step(self, batch, is_training: bool):
        """lightning.py:96-158."""
        prefix = "train" if is_training else "val"
        dry, wet, mod_sig, fx_params = batch
        if isinstance(self.model, RandomLFO):
            mod_sig_hat = self.model(wet.size(0), fx_params).to(wet.device)
        elif self.use_dry:
            assert dry is not None
            mod_sig_hat, _ = self.model(stack_dry_wet(dry, wet))
        else:
            mod_sig_hat, _ = self.model(wet)
        mod_sig_hat = mod_sig_hat.squeeze(1)
        lfo_sr = mod_sig_hat.size(-1) * float(self.sr) / wet.size(-1)       # the rate of the LFO's points (before any crop)
        if mod_sig is None:
            mod_sig = torch.zeros_like(mod_sig_hat)
        else:
            mod_sig = linear_interpolate_last_dim(mod_sig, mod_sig_hat.size(-1), align_corners=True)
        assert mod_sig.shape == mod_sig_hat.shape
        if self.model_smooth_n_frames > 1:
            if mod_sig_hat.requires_grad:       # training with smoothing (no shipped config): the kernel and its transpose as one autograd node
                mod_sig_hat = smoothen_with_grad(mod_sig_hat, self.model_smooth_n_frames)
            else:
                mod_sig_hat = smoothen(mod_sig_hat, self.model_smooth_n_frames)
            mod_sig = self.center_crop_mod_sig(mod_sig, mod_sig_hat.size(-1))
        if self.should_stretch:
            mod_sig_hat = stretch_corners(mod_sig_hat.detach(), max_n_corners=self.max_n_corners,
                                          smooth_n_frames=self.stretch_smooth_n_frames)
            if self.stretch_smooth_n_frames > 1:
                mod_sig = self.center_crop_mod_sig(mod_sig, mod_sig_hat.size(-1))
        assert mod_sig.shape == mod_sig_hat.shape
        loss = self.calc_and_log_losses(mod_sig_hat, mod_sig.contiguous(), self.loss_dict, f"{prefix}/")
        data_dict = {"wet": wet.detach(), "mod_sig": mod_sig.detach(), "mod_sig_hat": mod_sig_hat.detach()}
        if dry is not None:
            data_dict["dry"] = dry.detach()
        if self.fit_metrics is not None and not is_training:
            data_dict["lfo_fit"] = self._fit_and_log(mod_sig_hat, mod_sig, lfo_sr)
        return loss, data_dict, fx_params

    def sub_batch_size_common_step(self, batch, is_training: bool):
        """lightning.py:160-185."""
        dry, wet, mod_sig, fx_params = batch
        bs = mod_sig.size(0)
        assert bs >= self.sub_batch_size and bs % self.sub_batch_size == 0
        losses, out = [], None
        for s in range(0, bs, self.sub_batch_size):
            e = s + self.sub_batch_size
            sub = (None if dry is None else dry[s:e], wet[s:e], mod_sig[s:e],
                   {k: v[s:e] for k, v in fx_params.items()})
            out = self.common_step(sub, is_training=is_training)
            losses.append(out[0])
        return torch.stack(losses, dim=0).mean(dim=0), out[1], out[2]

    def training_step(self, batch, batch_idx: int = 0) -> T:
        step = self.common_step if self.sub_batch_size is None else self.sub_batch_size_common_step
        return step(batch, is_training=True)[0]

    def validation_step(self, batch, batch_idx: int = 0):
        step = self.common_step if self.sub_batch_size is None else self.sub_batch_size_common_step
        with torch.no_grad():
            return step(batch, is_training=False)


class _EffectAudioLossFn(torch.autograd.Function):
    """loss = sum_k w_k loss_k(effect(dry, mod_sig_hat), wet) as ONE autograd node for every ``effect``: ``forward(ctx,
    mod_sig_hat, step, dry, wet, consts, terms, *params)`` returns (loss, wet_hat (B, N)) and fills ``terms`` with the
    unweighted value of every weighted loss.  Every family renders its rows into one wet_hat (``step._render_rows``), the
    value-and-gradient kernels of the weighted losses run once (``effect_loss_grad``), and every family's adjoint writes its
    rows of one (B, n_frames) gradient at once (``step._adjoint_rows``).  Only that gradient (and those of ``params``) is
    kept for the backward, which scales it; d loss / d wet_hat, the stashes (allocated for all B rows) and the adjoints'
    workspaces do not outlive the call."""

    @staticmethod
    def forward(ctx, mod_sig_hat, step, dry, wet, consts, terms, *params):
        """``params``: the differentiable inputs beside the LFO, whose values ``consts`` already hold -- ``()``; ``(raw,)`` of
        ``step.learned_fx``; ``(latent, weight, bias)`` of ``step.fx_head`` (``step._head_rows``: what its forward launch kept).
        With them every family's adjoint is also asked for the per-clip fp64 gradients of its learned slots, rows of one
        (6, B) buffer, which ``mx_fx_params_grad`` reduces to d loss / d raw or ``mx_fx_head_bwd`` to the gradients of the
        three; without them the launches are those of the step without learned parameters."""
        from .effect_losses import effect_loss_grad, effect_loss_terms
        mod = mod_sig_hat.detach().float().contiguous()
        wet_hat, stashes = step._render_rows(dry, mod, consts, stash=True)
        rendered = wet_hat                        # what the adjoints (and the gain / FIR match's backward) read
        weighted: Dict[str, T] = {}
        P = step._warmup(dry.size(1))
        if P:                                     # the warm-up window: match and losses on columns [P:], dy zero on [:P]
            dy, wet_hat, a, t = _EffectAudioLossFn._windowed(step, rendered, wet, P, weighted)
        else:
            if step._matched:
                # every row in one launch sequence, dry rows included: the losses see the match
                wet_hat = step._match_rows(rendered, wet)
            a, t = wet_hat.unsqueeze(1), wet.unsqueeze(1)
            dy = effect_loss_grad(a, t, step.audio_loss_dict, values=weighted, **step._grad_modules())
            if step.match_shaper is not None:     # d loss / d (shaped rows) -> d loss / d (the linearly matched rows), in place
                from .shaper import match_shaper_backward
                match_shaper_backward(dy, step._shaper_in, wet, step._shaper, step.match_shaper_even, step.match_shaper_ridge,
                                      out=dy)
                step._shaper_in = None            # a batch-sized buffer: not kept between steps
            if step.match_gain is not None:       # d loss / d z -> d loss / d (the un-matched render), in place
                from .gain import match_gain_backward
                match_gain_backward(dy, rendered, wet, step._gain, step.match_gain, step.match_gain_eps, out=dy)
            if step.match_fir is not None:        # likewise, into a buffer of its own: a sample reads its neighbours' dz
                from .fir_match import match_fir_backward
                dy = match_fir_backward(dy, rendered, wet, step._fir, step.match_fir_ridge, step.match_fir_eps,
                                        step.match_fir_centre)
        # the adjoints write (they do not add) the rows of their family, and the reduction reads only those: no zeros
        gbuf = torch.empty((6, dry.size(0)), device=dry.device, dtype=torch.float64) if params else None
        dmod = step._adjoint_rows(dy, dry, mod, consts, stashes, gbuf=gbuf)
        param_grads: Tuple[Optional[T], ...] = ()
        if params:
            m = step._mixed_rows(dry.size(0), dry.device)
            geometry = (m["row_kind"], m["max_lfo_delay"], m["max_min_delay"])
            if step.fx_head is None:
                param_grads = (step.learned_fx.grad(gbuf, *geometry),)
            else:                               # (d_bias, d_weight, d_latent), reversed into the order of ``params``
                latent, (pooled, raw_rows) = params[0], step._head_rows
                param_grads = step.fx_head.backward_rows(gbuf, raw_rows, pooled, *geometry, latent.size(-1),
                                                         need_d_latent=latent.requires_grad)[::-1]
        ctx.save_for_backward(dmod, *param_grads)
        w = {k: v for k, v in step.audio_loss_dict.items() if v > 0}
        terms.update({k: v / w[k] for k, v in weighted.items()})
        if any(k in w for k in ("l1", "mse", "esr", "dc")):
            terms.update({k: v for k, v in effect_loss_terms(a, t).items() if k in w})
        ctx.mark_non_differentiable(wet_hat)
        return step.weighted_sum(terms, step.audio_loss_dict), wet_hat

    @staticmethod
    def _windowed(step, rendered, wet, P, weighted):
        """The match and the losses with a warm-up of P samples (``step.warmup_ms``): (d loss / d (the un-matched render) (B, N),
        wet_hat (B, N), and the (B, 1, N - P) pair the losses saw).  The match, the losses and the match's backward work on
        columns [P:] of every row -- views whose rows stay N floats apart, read in place -- and the gradient is zero on [:P].
        wet_hat holds the matched rows on [P:] (the match writes them there) and the un-matched render on [:P].  Without a
        match the loss kernels' dense (B, N - P) gradient is copied once into the (B, N) buffer the adjoints read."""
        from .effect_losses import effect_loss_grad
        seen, target = rendered[:, P:], wet[:, P:]
        wet_hat = rendered
        if step._matched:
            wet_hat = torch.empty_like(rendered)
            wet_hat[:, :P] = rendered[:, :P]
            step._match_rows(seen, target, out=wet_hat[:, P:])
        a, t = wet_hat[:, P:].unsqueeze(1), target.unsqueeze(1)
        dz = effect_loss_grad(a, t, step.audio_loss_dict, values=weighted, **step._grad_modules())
        dy = torch.empty_like(rendered)
        dy[:, :P] = 0.0
        if step.match_shaper is not None:         # first the curve's backward: in place on the dense dz when a linear match
            from .shaper import match_shaper_backward       # follows, else straight into the window of dy
            linear = step.match_gain is not None or step.match_fir is not None
            match_shaper_backward(dz, step._shaper_in, target, step._shaper, step.match_shaper_even, step.match_shaper_ridge,
                                  out=dz if linear else dy[:, P:])
            step._shaper_in = None                # a batch-sized buffer: not kept between steps
            if not linear:
                return dy, wet_hat, a, t
        if step.match_gain is not None:
            from .gain import match_gain_backward
            match_gain_backward(dz, seen, target, step._gain, step.match_gain, step.match_gain_eps, out=dy[:, P:])
        elif step.match_fir is not None:
            from .fir_match import match_fir_backward
            match_fir_backward(dz, seen, target, step._fir, step.match_fir_ridge, step.match_fir_eps, step.match_fir_centre,
                               out=dy[:, P:])
        else:
            dy[:, P:] = dz
        return dy, wet_hat, a, t

    @staticmethod
    def backward(ctx, g, _g_wet_hat):
        need = ctx.needs_input_grad               # of (mod_sig_hat, step, dry, wet, consts, terms, *params)
        dmod, *param_grads = ctx.saved_tensors
        d_params = tuple(t * g if t is not None and n else None for t, n in zip(param_grads, need[6:]))
        return (dmod * g if need[0] else None, None, None, None, None, None) + d_params


EFFECTS = ("flanger", "tremolo", "phaser")              # what a string ``effect`` may name
MIXED_KINDS = ("flanger", "chorus", "phaser", "tremolo", "dry")


def mixed_row_lists(kinds: Sequence[str], bs: int) -> Dict[str, List[int]]:
    """The rows of a batch of ``bs`` clips each launch family works on, by the batcher's rule (row i is of kind
    ``kinds[i % len(kinds)]``, data_modules.SyntheticFxBatcher, datasets.py:79-83): "delay" = flanger and chorus (one
    kernel, per-row geometry), "tremolo", "phaser", "dry".  A family without a row has an empty list."""
    family = {"flanger": "delay", "chorus": "delay", "tremolo": "tremolo", "phaser": "phaser", "dry": "dry"}
    out: Dict[str, List[int]] = {"delay": [], "tremolo": [], "phaser": [], "dry": []}
    for i in range(bs):
        out[family[kinds[i % len(kinds)]]].append(i)
    return out


# The per-row constants of the effect launches (the keys of fx.FX_CONSTS), in the order of the dict ``clip_constants`` returns:
# (key, the ``fx_params`` name it comes from, the launch families whose rows read it, its transform).  A key is present iff
# one of its families has a row.  Transform: None = the value itself, "1-" = 1 - v, else the per-row sample count of
# ``_mixed_rows`` the value is multiplied by.
CLIP_CONSTS = (("mix", "mix", ("delay", "tremolo", "phaser"), None),
               ("one_minus_mix", "mix", ("delay", "tremolo"), "1-"),
               ("feedback", "feedback", ("delay", "phaser"), None),
               ("depth", "depth", ("delay", "phaser"), None),
               ("lfo_scale", "width", ("delay",), "max_lfo_delay"),
               ("min_delay", "min_delay_width", ("delay",), "max_min_delay"),
               ("centre_frequency_hz", "centre_frequency_hz", ("phaser",), None))


class LFOExtractionThroughEffect(BaseLightingModule):
    """Trains the LFO extractor on dry / wet pairs WITHOUT an LFO label: the extractor's LFO drives a differentiable
    effect on ``dry`` and an audio-domain loss compares the result with ``wet``.  The reference has no such step
    (its lightning.py:65-199 trains against the ground-truth LFO only; its flanger, fx.py:72-119, has no usable autograd).

    Same batch 4-tuple ``(dry, wet, mod_sig, fx_params)`` and metric naming as ``LFOExtraction``; ``training_step`` returns a
    loss with a grad graph, so ``trainer.Trainer`` drives it unchanged.
    * ``effect``: "flanger" (flanger / chorus, the default), "tremolo" or "phaser" = that effect on every row; or a
      sequence of kinds out of "flanger", "chorus", "phaser", "tremolo", "dry" = a batch that mixes them: row i is of kind
      ``effect[i % len(effect)]``, the batcher's own rule (``data_modules.SyntheticFxBatcher``, datasets.py:79-83), so
      ``InterwovenDataModule`` batches and each DDP rank's local batch line up with ``effect=("flanger", "chorus",
      "phaser")``.  A string is the sequence of that one kind: there is ONE path.  Every launch family (flanger + chorus;
      tremolo; phaser) renders its rows into one shared wet_hat and its adjoint writes its rows of one shared gradient
      through the kernels' row lists (``_render_rows`` / ``_adjoint_rows``); a family that owns every row is launched
      without a list.  "dry" rows are copied and get a zero gradient.  The caveats below apply row by row.
    * ``max_min_delay_ms`` / ``max_lfo_delay_ms``: the geometry of the "flanger" rows (with ``effect="flanger"``: ONE flanger
      or chorus geometry per module, as in ``fx.MonoFlangerChorusModule``); ignored without such a row.
      ``chorus_max_min_delay_ms`` / ``chorus_max_lfo_delay_ms`` (default ``data_modules.CHORUS_FX``: 30 ms / 10 ms): the
      geometry of the "chorus" rows of a sequence.  The tremolo and the phaser have no delay-line limit.
    * ``fx_params`` carries what the kinds present need, each as ONE (B,) tensor over all rows (the batcher's merged
      ``depth`` / ``feedback`` / ``mix``) or a python float: the flanger and chorus ``feedback``, ``min_delay_width``,
      ``width``, ``depth``, ``mix``; the tremolo only ``mix``; the phaser ``depth``, ``centre_frequency_hz``, ``feedback``,
      ``mix`` (its ``rate_hz`` and ``lead`` are ignored: the LFO is the extractor's)
      (``check_fx_params``: range-check them on every step, which costs host synchronisations).
    * ``audio_loss_dict``: names from ``effect_losses.GRAD_NAMES``; zero-weight names are only logged.
    * ``pre_emph_filter_cfs`` / ``pre_emph_low_pass``: the filter of the "esr_pre" loss (``losses.PreEmphESRLoss``; 1 .. 16
      taps), ignored without that name.
    * ``learned_fx`` (optional): a spec dict or an ``fx.LearnedFxParams`` -- effect parameters fitted together with the
      extractor, ONE shared value per (kind, name), each mapped onto its valid range; a bare number in the spec fixes a
      parameter.  A learned or fixed (kind, name) overrides the batch's ``fx_params`` on the rows of that kind, every other
      name is read from the batch; a name that a present kind needs and nobody supplies raises a ``ValueError`` naming it,
      so with every name covered the step trains on ``(dry, wet, None, None)`` batches (recorded pairs).  The mapped
      values are written into the per-row constants by ``mx_fx_params_expand`` and d loss / d raw comes from the adjoints'
      per-clip parameter gradients through ``mx_fx_params_grad``; ``learned_fx.raw`` is an ordinary parameter (optimizer,
      DDP, checkpoints), AdamW's weight decay pulls a value towards the middle of its range, and every training step logs
      ``fx/<kind>.<name>``.  ``render`` and validation use the learned values.  The default adds no parameter and leaves
      the step's launches as they are.  What a fit cannot tell apart (``width`` and the LFO's amplitude, ``min_delay_width``
      and its offset, the flanger's ``mix * depth``): DESIGN section 7.
    * ``fx_head`` (optional, not together with ``learned_fx``): a spec dict (the grammar of ``learned_fx``, plus the optional
      keys ``in_ch`` and ``raw_gain`` beside the kinds) or an ``fx.FxParamHead`` -- effect parameters PER CLIP, predicted by one
      linear layer on the mean over time of the model's latent, the second output of ``Spectral2DCNN.forward`` (B, in_ch,
      n_frames); a model without it raises a ``ValueError``.  Precedence, fixed values, coverage and errors are those of
      ``learned_fx``.  ``mx_fx_head_fwd`` writes the predicted values into the per-row constants, ``mx_fx_head_bwd`` turns the
      adjoints' per-clip parameter gradients into the gradients of ``fx_head.weight`` / ``fx_head.bias`` (ordinary
      parameters) and of the latent, which reaches the CNN's backward beside d loss / d LFO.  A fresh head (zero weight)
      is ``learned_fx`` at its ``init``.  Every training step logs ``fx/<kind>.<name>`` = the mean of the predicted values
      over the rows of that kind and ``fx_std/<kind>.<name>`` = their standard deviation; ``data_dict["fx_values"]`` holds
      them all, (B, P).  ``render(..., latent=)`` needs the latent.
    * ``match_gain`` (optional): "ls" or "rms" -- one gain per clip that carries the re-render onto ``wet`` before any loss
      sees it (``gain.match_gain``, K20: "ls" the least-squares gain <wet_hat, wet> / (<wet_hat, wet_hat> + eps), "rms" the
      energy match), with ``match_gain_eps`` and the clamp ``match_gain_range`` = (lo, hi), 0 < lo <= 1 <= hi, or None.
      A recorded wet is never at the dry's level and every effect here passes the dry at unit gain.  All rows of the batch
      are matched in one launch pair, the losses, the returned ``wet_hat`` and the logged terms are those of the matched
      rows, and d loss / d wet_hat passes through ``gain.match_gain_backward`` (in place) before the adjoints, which read the
      un-matched render.  A training step logs ``gain/mean``, ``gain/std`` and ``gain/clamped`` (the share of clamped rows),
      ``data_dict["gain"]`` is the (B,) vector; ``render`` has no ``wet`` and stays un-matched.  Without it the step's
      launches are unchanged.  What a free gain trades off against: DESIGN section 7.
    * ``match_fir`` (optional, not together with ``match_gain``): K in 1 .. 32 -- one K-tap least-squares FIR per clip, fitted
      from the re-render onto ``wet`` before any loss sees it (``fir_match.match_fir``, K21), with the centre
      ``match_fir_centre`` (None: (K - 1) // 2), ``match_fir_ridge``, ``match_fir_eps`` and the guard ``match_fir_max_gain`` on
      sum |h|.  It absorbs what a recording chain adds to a wet: a level (K = 1 is the "ls" gain), a tone curve, and a lag
      of a fraction of a sample.  It sits exactly where ``match_gain`` sits: all rows in one launch sequence before the
      losses; the losses, the returned ``wet_hat`` and the logged terms are those of the matched rows; d loss / d z passes
      through ``fir_match.match_fir_backward`` (into a buffer of its own) before the adjoints, which read the un-matched
      render; ``render`` stays un-matched.  A training step logs ``fir/dc_gain`` (mean of sum_k h), ``fir/l1`` (mean of
      sum |h|) and ``fir/flagged`` (the share of rows a guard gave the identity filter); ``data_dict["fir"]`` is the (B, K)
      taps.  Without it the step's launches are unchanged.  What the match is not, and the identifiability limit on
      K - 1 - centre: DESIGN section 7, "Tone and sub-sample lag of recorded pairs".
    * ``warmup_ms`` (optional): a loss warm-up window of P = ``fx.delay_samples(warmup_ms, sr)`` samples for chunks cut from
      the inside of a recording, whose ``wet`` had the samples before the chunk in its delay line or filter state while the
      re-render starts empty.  The extractor sees the whole clip and every row is rendered over all N samples as before;
      everything that compares with ``wet`` -- the gain / FIR match (partials, solve, apply, and its backward), the loss
      gradients, the logged terms, validation -- works on columns [P:] of every row (views, rows N apart; the FIR's "zeros
      outside" means outside the view).  d loss / d wet_hat is zero on [:P] and the adjoints run on all N samples of the
      un-matched render, so LFO frames inside the warm-up get gradient only through what they leave in the effect's state.
      ``wet_hat`` stays (B, 1, N): [P:] the matched rows, [:P] the un-matched render; ``data_dict["warmup"]`` = P.  A step
      whose losses would see P samples or fewer raises a ``ValueError``.  One P per module; ``render`` is unchanged.  None,
      or a value that gives P = 0, is the step without it.  How large P must be: DESIGN section 7, "Warm-up of a chunk cut
      from a file".
    * ``match_shaper`` (optional, alone or together with ``match_gain`` or ``match_fir``): the order P in 1 .. 7 of one
      memoryless polynomial curve per clip, fitted from the (linearly matched) re-render onto ``wet`` before any loss sees
      it (``shaper.match_shaper``, K27), with ``match_shaper_even`` (the even powers too, for asymmetric curves),
      ``match_shaper_ridge`` and the guard ``match_shaper_max_gain`` on sum |c|.  It absorbs what a compander, an op-amp
      stage or a re-amp box does to the peaks of a recorded wet.  The linear match runs first and the curve is fitted on its
      rows, aligned and at the level of ``wet``; the losses, the returned ``wet_hat``, the logged terms and validation see
      the shaped rows; d loss / d z passes through ``shaper.match_shaper_backward`` (in place; it reads the linear match's
      rows and ``wet``), then through the linear match's backward, then into the adjoints, which read the un-matched render;
      under ``warmup_ms`` all of it works on columns [P:].  A training step logs ``shaper/linear`` (mean c_1),
      ``shaper/curve`` (mean of sum_{k >= 2} |c_k|) and ``shaper/flagged``; ``data_dict["shaper"]`` is the (B, K)
      coefficients; ``render`` stays un-matched.  Without it the step's launches are unchanged.  What the match is not:
      DESIGN section 7, "Saturation of recorded pairs".
    * ``loss_dict`` (optional, default none): an LFO-domain term (lightning.py:33-62) added to the loss when the batch carries
      ``mod_sig``; it is logged as ``{prefix}/lfo_{name}``.
    The LFO enters the effect at the extractor's own rate (n_frames points, resampled in-kernel exactly as the data path
    resamples its n_samples // 100 label), so for the flanger and the tremolo a re-render from the label the batch was rendered with is bit-identical to
    ``wet`` and every loss is exactly 0 there.

    ``model_smooth_n_frames`` > 1 applies the moving average (with its transpose in the backward) and centre-crops dry and
    wet by the rule of ``TBPTTLFOEffectModeling._prepare_all_rows``.  One limit of that crop: the re-render starts from an
    EMPTY delay line at the first cropped sample, whereas the recorded wet had the samples before the crop in its line, so
    the first ``max_delay_samples`` samples of ``wet_hat`` differ from ``wet`` even for the true LFO (with feedback: longer).
    ``warmup_ms`` leaves those samples out of every comparison; without it the default is therefore no smoothing.  The
    tremolo has no state, so this caveat does not apply to it: the re-render of a cropped clip does not depend on the
    samples before the crop.

    The phaser's lead-in rule: the step re-renders from ``dry`` ALONE, with lead 0 and empty filter state
    (``mx_phaser_fwd_stash`` on the LFO expanded by ``mx_phaser_mod_expand``).  The batch's ``wet`` was rendered by JUCE's
    oscillator after ``fx_params["lead"]`` warm-up samples, which the batch tuple does not carry -- in the reference and the
    data path that lead exists to randomise the LFO's phase.  So at the true label the loss is small but NOT exactly 0, for
    three reasons: the start transient of the six all-passes and the feedback path; a cut-off-update grid shifted by
    ``lead % 4`` samples against the recorded one; and a label that is the sine linearly interpolated from
    ``n_samples // 100`` points.  The same kind of caveat as the flanger's crop above; ``warmup_ms`` removes the first of the
    three from the comparison (the start transient), not the other two.

    ``should_stretch`` is not wired in (the corner stretch has a backward, but not on this path)."""
    default_audio_loss_dict = {"mrstft": 1.0}

    def __init__(self,
                 model: nn.Module,
                 sr: float = 44100,
                 use_dry: bool = True,
                 model_smooth_n_frames: int = 0,
                 max_min_delay_ms: float = 1.0,
                 max_lfo_delay_ms: float = 10.0,
                 audio_loss_dict: Optional[Dict[str, float]] = None,
                 loss_dict: Optional[Dict[str, float]] = None,
                 should_stretch: bool = False,
                 check_fx_params: bool = False,
                 effect: Union[str, Sequence[str]] = "flanger",
                 chorus_max_min_delay_ms: Optional[float] = None,
                 chorus_max_lfo_delay_ms: Optional[float] = None,
                 pre_emph_filter_cfs: Sequence[float] = (-0.95, 1.0),
                 pre_emph_low_pass: bool = False,
                 learned_fx=None,
                 fx_head=None,
                 match_gain: Optional[str] = None,
                 match_gain_eps: float = 1e-8,
                 match_gain_range: Optional[Sequence[float]] = (0.05, 20.0),
                 match_fir: Optional[int] = None,
                 match_fir_centre: Optional[int] = None,
                 match_fir_ridge: float = 1e-6,
                 match_fir_eps: float = 1e-8,
                 match_fir_max_gain: float = 20.0,
                 warmup_ms: Optional[float] = None,
                 match_shaper: Optional[int] = None,
                 match_shaper_even: bool = False,
                 match_shaper_ridge: float = 1e-9,
                 match_shaper_max_gain: float = 20.0) -> None:
        super().__init__({} if loss_dict is None else loss_dict)
        self._set_pre_emph(pre_emph_filter_cfs, pre_emph_low_pass)
        from . import fx
        if warmup_ms is not None and (isinstance(warmup_ms, bool) or not isinstance(warmup_ms, (int, float))
                                      or not 0.0 <= warmup_ms < float("inf")):
            raise ValueError(f"warmup_ms must be None or a finite number >= 0, got {warmup_ms!r}")
        self.warmup_ms = warmup_ms
        self.warmup_samples = 0 if warmup_ms is None else fx.delay_samples(warmup_ms, sr)    # P; 0 = the step without it
        from .fir_match import check_fir
        from .gain import check_mode
        # validated without match_fir too, as the gain's arguments are (a centre is checked against the taps it belongs to)
        _, fir_centre, _, _, _ = check_fir(1 if match_fir is None else match_fir, None if match_fir is None else match_fir_centre,
                                           match_fir_ridge, match_fir_eps, match_fir_max_gain, "match_fir")
        if match_fir is None and match_fir_centre is not None and (
                isinstance(match_fir_centre, bool) or not isinstance(match_fir_centre, int) or match_fir_centre < 0):
            raise ValueError(f"match_fir: centre must be an integer in 0 .. taps - 1 (or None), got {match_fir_centre!r}")
        if match_fir is not None and match_gain is not None:
            raise ValueError("match_fir and match_gain are mutually exclusive: one tap of the FIR match is the ls gain")
        self.match_fir = match_fir
        self.match_fir_centre = fir_centre if match_fir is not None else match_fir_centre
        self.match_fir_ridge, self.match_fir_eps, self.match_fir_max_gain = match_fir_ridge, match_fir_eps, match_fir_max_gain
        self._fir = None                        # the fir_match.FirMatch of the last matched batch
        if isinstance(match_gain_range, list):  # a config file's spelling of the pair
            match_gain_range = tuple(match_gain_range)
        # eps and the range are validated without match_gain too: a typo does not wait for the day it is switched on
        check_mode("ls" if match_gain is None else match_gain, match_gain_eps, match_gain_range, "match_gain")
        self.match_gain, self.match_gain_eps, self.match_gain_range = match_gain, match_gain_eps, match_gain_range
        self._gain = None                       # the gain.GainMatch of the last matched batch
        from .shaper import check_shaper
        # validated without match_shaper too, as the gain's and the FIR's arguments are
        check_shaper(5 if match_shaper is None else match_shaper, match_shaper_even, match_shaper_ridge, match_shaper_max_gain,
                     "match_shaper")
        self.match_shaper, self.match_shaper_even = match_shaper, match_shaper_even
        self.match_shaper_ridge, self.match_shaper_max_gain = match_shaper_ridge, match_shaper_max_gain
        self._shaper = None                     # the shaper.ShaperMatch of the last matched batch
        self._shaper_in = None                  # the rows it was fitted on (the linear match's z, or the render itself), from
                                                # _match_rows until the curve's backward has read them
        self._matched = match_gain is not None or match_fir is not None or match_shaper is not None
        from .effect_losses import GRAD_NAMES
        if should_stretch:
            raise NotImplementedError("should_stretch is not supported when training through the rendered effect")
        self.kinds: Optional[Tuple[str, ...]] = None                # a sequence ``effect``: the kind of every slot
        if not isinstance(effect, str):
            self.kinds = effect = tuple(effect)
            if not effect:
                raise ValueError("effect: an empty sequence of kinds")
            for k in effect:
                if k not in MIXED_KINDS:
                    raise ValueError(f"effect kind '{k}': supported are {MIXED_KINDS}")
        elif effect not in EFFECTS:
            raise ValueError(f"effect '{effect}': supported are {EFFECTS} or a sequence out of {MIXED_KINDS}")
        self.effect = effect
        self._kinds: Tuple[str, ...] = (effect,) if self.kinds is None else self.kinds      # the slots every step goes by
        audio_loss_dict = dict(self.default_audio_loss_dict if audio_loss_dict is None else audio_loss_dict)
        for name, w in audio_loss_dict.items():
            if w > 0 and name not in GRAD_NAMES:
                raise NotImplementedError(f"audio loss '{name}' has no gradient kernel (supported: {GRAD_NAMES})")
        if not any(w > 0 for w in audio_loss_dict.values()):
            raise ValueError("audio_loss_dict needs at least one loss with a weight above 0")
        self.max_min_delay_samples = self.max_lfo_delay_samples = 0   # no delay line: the arguments are ignored
        if "flanger" in self._kinds:
            self.max_min_delay_samples, self.max_lfo_delay_samples = self._delay_line(max_min_delay_ms, max_lfo_delay_ms, sr, "")
        self.max_delay_samples = self.max_min_delay_samples + self.max_lfo_delay_samples
        if self.kinds is not None:
            from .data_modules import CHORUS_FX
            if chorus_max_min_delay_ms is None:
                chorus_max_min_delay_ms = CHORUS_FX["max_min_delay_ms"]
            if chorus_max_lfo_delay_ms is None:
                chorus_max_lfo_delay_ms = CHORUS_FX["max_lfo_delay_ms"]
            self.chorus_max_min_delay_ms, self.chorus_max_lfo_delay_ms = chorus_max_min_delay_ms, chorus_max_lfo_delay_ms
            self.chorus_max_min_delay_samples = self.chorus_max_lfo_delay_samples = 0
            if "chorus" in self.kinds:
                self.chorus_max_min_delay_samples, self.chorus_max_lfo_delay_samples = self._delay_line(
                    chorus_max_min_delay_ms, chorus_max_lfo_delay_ms, sr, "chorus_")
        self.model = model
        self.sr, self.use_dry = sr, use_dry
        self.model_smooth_n_frames = model_smooth_n_frames
        self.max_min_delay_ms, self.max_lfo_delay_ms = max_min_delay_ms, max_lfo_delay_ms
        self.check_fx_params = check_fx_params
        self.audio_loss_dict = audio_loss_dict
        # the base class holds the LFO-domain term; loss_dict names every metric this step logs (trainer.metric_names)
        self.lfo_loss_dict = self.loss_dict
        self.loss_dict = dict(audio_loss_dict, **{f"lfo_{k}": w for k, w in self.lfo_loss_dict.items()})
        self._mixed = None
        learned_fx = self._param_source(learned_fx, "learned_fx", fx.LearnedFxParams)
        self.learned_fx = learned_fx                                # None registers nothing: the parameters are the model's
        if fx_head is not None and learned_fx is not None:
            raise ValueError("learned_fx and fx_head are mutually exclusive: shared and per-clip entries do not mix")
        self.fx_head = fx_head = self._param_source(fx_head, "fx_head", fx.FxParamHead, ("in_ch", "raw_gain"))     # likewise
        self._fixed_plan = None
        self._fx_values: Optional[T] = None
        self._head_rows: Optional[Tuple[T, T]] = None               # (pooled, raw_rows) of the last mx_fx_head_fwd
        # the scalars ``common_step`` logs per training step beside the losses (trainer.metric_names)
        self.step_metric_names = [] if learned_fx is None else [f"fx/{n}" for n in learned_fx.names]
        if fx_head is not None:
            self.step_metric_names = [f"fx/{n}" for n in fx_head.names] + [f"fx_std/{n}" for n in fx_head.names]
        if match_gain is not None:
            self.step_metric_names = self.step_metric_names + ["gain/mean", "gain/std", "gain/clamped"]
        if match_fir is not None:
            self.step_metric_names = self.step_metric_names + ["fir/dc_gain", "fir/l1", "fir/flagged"]
        if match_shaper is not None:
            self.step_metric_names = self.step_metric_names + ["shaper/linear", "shaper/curve", "shaper/flagged"]

    def _match_rows(self, rendered: T, wet: T, out: Optional[T] = None) -> T:
        """The rows of ``rendered`` brought to the level of ``wet`` (``gain.match_gain``: two launches for all rows) or to its
        level, tone and sub-sample lag (``fir_match.match_fir``: three); the ``GainMatch`` / ``FirMatch`` is kept in ``_gain``
        / ``_fir`` for the backward, the log and ``data_dict``.  ``out``: where the matched rows go (the warm-up window: a view
        of the step's wet_hat).  With ``match_shaper`` the linear match (if any) runs first, into a buffer of its own, and the
        curve (``shaper.match_shaper``, K27: three calls) is fitted on its rows -- aligned and at the level of ``wet``; the
        ``ShaperMatch`` is kept in ``_shaper`` and the rows it read in ``_shaper_in``."""
        kw = {} if out is None else {"out": out}
        if self.match_shaper is None:
            return self._match_linear(rendered, wet, kw)
        from .shaper import match_shaper
        linear = self.match_gain is not None or self.match_fir is not None
        self._shaper_in = self._match_linear(rendered, wet, {}) if linear else rendered
        self._shaper = match_shaper(self._shaper_in, wet, self.match_shaper, self.match_shaper_even, self.match_shaper_ridge,
                                    self.match_shaper_max_gain, **kw)
        return self._shaper.z

    def _match_linear(self, rendered: T, wet: T, kw) -> T:
        """The gain or the FIR match of ``_match_rows``; ``kw``: its ``out``, if any."""
        if self.match_fir is not None:
            from .fir_match import match_fir
            self._fir = match_fir(rendered, wet, self.match_fir, self.match_fir_centre, self.match_fir_ridge,
                                  self.match_fir_eps, self.match_fir_max_gain, **kw)
            return self._fir.z
        from .gain import match_gain
        self._gain = match_gain(rendered, wet, self.match_gain, self.match_gain_eps, self.match_gain_range, **kw)
        return self._gain.z

    def _warmup(self, n: int) -> int:
        """P, the samples every comparison with ``wet`` leaves out, for rows of ``n`` samples (after the smoothing crop), or the
        ValueError when nothing would be left."""
        if self.warmup_samples >= n:
            raise ValueError(f"warmup_ms = {self.warmup_ms} is {self.warmup_samples} samples, and the losses see rows of {n}: "
                             "nothing is left to compare")
        return self.warmup_samples

    @property
    def _fxp(self):
        """Who supplies learned / fixed effect parameters: ``learned_fx``, ``fx_head`` or None."""
        return self.learned_fx if self.learned_fx is not None else self.fx_head

    @staticmethod
    def _delay_line(max_min_delay_ms: float, max_lfo_delay_ms: float, sr: float, prefix: str) -> Tuple[int, int]:
        """The two sample counts of the delay-line geometry ``{prefix}max_min_delay_ms`` / ``{prefix}max_lfo_delay_ms``
        (``prefix``: "" for the flanger rows, "chorus_" for the chorus rows), or the ValueError that says what is wrong."""
        from . import fx
        if max_min_delay_ms < 0 or max_lfo_delay_ms < 0:
            raise ValueError(f"{prefix}max_min_delay_ms and {prefix}max_lfo_delay_ms must not be negative")
        n_min, n_lfo = fx.delay_samples(max_min_delay_ms, sr), fx.delay_samples(max_lfo_delay_ms, sr)
        if not 2 <= n_min + n_lfo <= fx.FLANGER_MAX_DELAY_SAMPLES:
            raise ValueError(f"{prefix.replace('_', ' ')}delay line of {n_min + n_lfo} samples: the flanger kernels keep it in LDS "
                             f"and support 2 .. {fx.FLANGER_MAX_DELAY_SAMPLES} samples (LFO row included)")
        return n_min, n_lfo

    def _param_source(self, arg, what: str, cls, own_keys: Sequence[str] = ()):
        """The ``learned_fx`` / ``fx_head`` argument (``what``) as its ``cls`` object: built from a spec dict (``own_keys``: the
        constructor's keywords that sit beside the kinds), type-checked, and naming none but this step's kinds.  None stays."""
        if isinstance(arg, dict):
            spec = dict(arg)
            own = {k: spec.pop(k) for k in own_keys if k in spec}
            arg = cls(spec, **own)
        if arg is not None:
            if not isinstance(arg, cls):
                raise ValueError(f"{what}: a spec dict or an fx.{cls.__name__}")
            for k in arg.kinds:
                if k not in self._kinds:
                    raise ValueError(f"{what} names the kind '{k}', which is not among this step's kinds {self._kinds}")
        return arg

    def _mixed_rows(self, bs: int, device) -> Dict[str, object]:
        """The row plan of a batch of ``bs`` rows on ``device`` (cached): the int32 row list of every launch family, the
        int64 list of the dry rows, the per-row delay-line geometry as the batcher forms it (``SyntheticFxBatcher.__init__``:
        fp32 sample counts, chorus rows the chorus geometry, every other row the flanger's; only the rows of the "delay"
        list are read), and "all_rows": the family that owns every row of the batch, if one does (else None)."""
        m = self._mixed
        if m is None or m["bs"] != bs or m["device"] != device:
            lists = mixed_row_lists(self._kinds, bs)
            kinds = [self._kinds[i % len(self._kinds)] for i in range(bs)]
            mm = torch.tensor([self.chorus_max_min_delay_samples if k == "chorus" else self.max_min_delay_samples
                               for k in kinds], dtype=torch.float32)
            ml = torch.tensor([self.chorus_max_lfo_delay_samples if k == "chorus" else self.max_lfo_delay_samples
                               for k in kinds], dtype=torch.float32)
            m = {"bs": bs, "device": device, "lists": lists,
                 "all_rows": next((f for f in ("delay", "tremolo", "phaser") if len(lists[f]) == bs > 0), None),
                 "max_min_delay": mm.to(device), "max_lfo_delay": ml.to(device),
                 "max_delay": (mm + ml).to(torch.int32).to(device),
                 "max_delay_max": int(max([int(mm[i] + ml[i]) for i in lists["delay"]], default=0)),
                 "dry_idx": torch.tensor(lists["dry"], dtype=torch.int64, device=device)}
            for name in ("delay", "tremolo", "phaser"):
                m[name] = torch.tensor(lists[name], dtype=torch.int32, device=device)
            if self._fxp is not None:                               # the kind code of every row (fx.FX_KINDS)
                from . import fx
                m["kinds"] = kinds
                m["row_kind"] = torch.tensor([fx.FX_KINDS.index(k) for k in kinds], dtype=torch.int32, device=device)
            if self.fx_head is not None:                            # (B, P): row b is of entry e's kind; rows per entry (>= 1)
                mask = torch.tensor([[float(k == n.split(".", 1)[0]) for n in self.fx_head.names] for k in kinds],
                                    dtype=torch.float32).view(bs, len(self.fx_head.names))
                m["head_mask"], m["head_count"] = mask.to(device), mask.sum(0).clamp(min=1.0).to(device)
            self._mixed = m
        return m

    @staticmethod
    def _launch_rows(m: Dict[str, object], family: str) -> Optional[T]:
        """The row list a family's launches get.  A family that owns every row gets None: by the kernels' row-list contract
        a listed row runs the very same code as without a list, so the bits are the same, and the launches, their arguments
        and the allocations of ``effect="flanger"`` / ``"tremolo"`` / ``"phaser"`` are those of the un-listed wrappers
        (``_render_rows`` / ``_adjoint_rows`` then allocate nothing themselves)."""
        return None if m["all_rows"] == family else m[family]

    def clip_constants(self, fx_params, bs: int, device, latent: Optional[T] = None) -> Dict[str, T]:
        """ONE dict of (B,) fp32 constants for all families of the batch: the keys of ``CLIP_CONSTS`` whose families have a
        row, in its order, read from ``fx_params`` or supplied by ``learned_fx`` / ``fx_head`` (precedence: the class docstring).
        The rounding rule is the data path's (``SyntheticFxBatcher.render``, ``fx.derive_clip_constants``), so a re-render from
        the label reproduces ``wet``: a tensor parameter meets the per-row sample count in fp32 and one_minus_mix is 1 - mix in
        fp32; a python float, and a number fixed by ``learned_fx`` / ``fx_head``, meets them in double and is rounded once; a
        learned or predicted value is mapped in fp64, rounded once and then follows the rule of a tensor parameter
        (``mx_fx_params_expand`` / ``mx_fx_head_fwd``, the one launch).  Only what the kinds present need is read from
        ``fx_params``; a ValueError names what nobody supplies.
        With ``learned_fx`` / ``fx_head`` the fixed numbers (``_fixed_vectors``) lie over the batch's vectors on the rows of their
        kind, the launch writes the learned values over the rows of theirs, and its (P,) / (B, P) fp32 values are kept for
        ``common_step`` to log (``fx_head``: also ``_head_rows``).  Without ``fx_params`` the vectors are the cached ones,
        rewritten in place on every step: no launch but the one.  ``latent`` (B, in_ch, W): what a step with ``fx_head``
        predicts from, required then."""
        from . import fx
        src = self._fxp
        self._require_fx_params(fx_params, bs)
        if self.fx_head is not None:
            if latent is None:
                raise ValueError("a step with fx_head predicts the effect parameters from the model's latent: pass latent=")
            latent = self._head_latent(latent, bs)
        m = self._mixed_rows(bs, device)
        if self.check_fx_params:                                    # what is read from the batch, each kind's ranges on its own rows
            kinds = [self._kinds[i % len(self._kinds)] for i in range(bs)]
            for kind in dict.fromkeys(kinds):
                rows = [i for i in range(bs) if kinds[i] == kind]
                for name in fx.FX_PARAM_NAMES.get(kind, ()):
                    if src is None or not src.covers(kind, name):
                        p = fx_params[name]
                        fx._check_range(p[rows] if isinstance(p, T) and len(rows) < bs else p, len(rows),
                                        *fx._fx_param_range(kind, name))
        plan = None if src is None else self._fixed_vectors(m)

        def transformed(v: T, how: Optional[str]) -> T:
            return v if how is None else 1.0 - v if how == "1-" else v * m[how]

        consts = {}
        for key, name, families, how in CLIP_CONSTS:
            if not any(m["lists"][f] for f in families):
                continue
            p = None if fx_params is None else fx_params.get(name)
            if p is None:                                           # learned / fixed on every row that reads it
                consts[key] = plan["vals"][key]
                continue
            if isinstance(p, T):
                assert p.shape == (bs,), f"fx_params['{name}']: a ({bs},) tensor or a python float"
                v = transformed(p.to(device=device, dtype=torch.float32), how)
            else:
                v = transformed(torch.full((bs,), float(p), device=device, dtype=torch.float64), how).float()
            if plan is not None:
                if plan["mask"][key] is not None:
                    v = torch.where(plan["mask"][key], plan["vals"][key], v)
                elif key in plan["learned"] and isinstance(p, T) and v.data_ptr() == p.data_ptr():
                    v = v.clone()                                   # the launch below writes: not into the batch's own tensor
            consts[key] = v.contiguous()
        if src is None:
            return consts
        geometry = (m["row_kind"], m["max_lfo_delay"], m["max_min_delay"])
        if self.fx_head is None:
            self._fx_values = src.expand(consts, *geometry)
        else:
            pooled, raw_rows, self._fx_values = src.forward_rows(latent, consts, *geometry)
            self._head_rows = (pooled, raw_rows)
        return consts

    def _fixed_vectors(self, m: Dict[str, object]) -> Dict[str, object]:
        """What ``learned_fx`` / ``fx_head`` fix or learn, laid out on the rows of the plan ``m``, per (B, device) once: "vals"
        the (B,) fp32 vector of every key of ``fx.FX_CONSTS`` (a fixed number on the rows of its kind, 0 elsewhere), "mask" its
        (B,) bool rows (None for a key without one), "learned" the keys the launch writes."""
        from . import fx
        src, bs, device, kinds = self._fxp, m["bs"], m["device"], m["kinds"]
        plan = self._fixed_plan
        if plan is None or plan["bs"] != bs or plan["device"] != device:
            counts = {k: m[k].double().cpu() for k in ("max_lfo_delay", "max_min_delay")}
            vals = {k: torch.zeros(bs, dtype=torch.float64) for k in fx.FX_CONSTS}
            mask = {k: torch.zeros(bs, dtype=torch.bool) for k in fx.FX_CONSTS}
            for (kind, name), v in src.fixed.items():
                for i in (i for i in range(bs) if kinds[i] == kind):
                    for key, from_name, _, how in CLIP_CONSTS:
                        if from_name == name:
                            vals[key][i] = v if how is None else 1.0 - v if how == "1-" else v * float(counts[how][i])
                            mask[key][i] = True
            learned = {n.split(".", 1)[1] for n in src.names}
            plan = {"bs": bs, "device": device, "vals": {k: v.float().to(device) for k, v in vals.items()},
                    "mask": {k: (v.to(device) if bool(v.any()) else None) for k, v in mask.items()},
                    "learned": {key for key, from_name, _, _ in CLIP_CONSTS if from_name in learned}}
            self._fixed_plan = plan
        return plan

    def missing_fx_params(self, fx_params, bs: int) -> List[str]:
        """The "<kind>.<name>" a batch of ``bs`` rows needs for its re-render and has from nowhere: not in ``fx_params`` (which
        may be None: a dry / wet pair of a recording) and neither learned nor fixed by ``learned_fx`` / ``fx_head``."""
        from . import fx
        out = []
        for kind in dict.fromkeys(self._kinds[i % len(self._kinds)] for i in range(bs)):
            for name in fx.FX_PARAM_NAMES.get(kind, ()):
                if (fx_params is None or name not in fx_params) and not (self._fxp is not None
                                                                         and self._fxp.covers(kind, name)):
                    out.append(f"{kind}.{name}")
        return out

    def _require_fx_params(self, fx_params, bs: int) -> None:
        """The ValueError that lists ``missing_fx_params``, if any."""
        missing = self.missing_fx_params(fx_params, bs)
        if missing:
            raise ValueError(f"the re-render needs {missing}: neither in the batch's fx_params nor learned / fixed through "
                             f"learned_fx or fx_head")

    def _head_latent(self, latent, bs: int) -> T:
        """The latent as ``mx_fx_head_fwd`` reads it, or the ValueError that says what is wrong with it."""
        if not (isinstance(latent, T) and latent.ndim == 3 and latent.size(0) == bs and latent.dtype == torch.float32):
            raise ValueError(f"fx_head needs the model's latent as a ({bs}, in_ch, n_frames) fp32 tensor")
        if latent.size(1) != self.fx_head.in_ch:
            raise ValueError(f"the model's latent has {latent.size(1)} channels, fx_head was built for in_ch = "
                             f"{self.fx_head.in_ch}")
        return latent.detach().contiguous()

    def _render_rows(self, dry: T, mod: T, consts: Dict[str, T], stash: bool):
        """wet_hat (B, N), every family through its row list (``_launch_rows``) into the one buffer: flanger + chorus rows
        ``mx_flanger_fwd`` (``stash``: ``mx_flanger_fwd_stash``, the same bits), tremolo rows ``mx_tremolo_fwd``, phaser rows
        ``mx_phaser_mod_expand`` + ``mx_phaser_fwd_stash`` with lead 0, dry rows a copy.  A family without a row launches
        nothing.  Returns (wet_hat, the stashes ``_adjoint_rows`` needs -- empty unless ``stash``)."""
        from . import fx
        B, N = dry.shape
        m = self._mixed_rows(B, dry.device)
        wet_hat = None if m["all_rows"] else torch.empty((B, N), device=dry.device, dtype=torch.float32)
        stashes = {}
        if m["dry_idx"].numel():
            wet_hat.index_copy_(0, m["dry_idx"], dry.index_select(0, m["dry_idx"]))
        if m["delay"].numel():
            geometry, rows = (m["max_delay"], m["max_delay_max"]), self._launch_rows(m, "delay")
            if stash:
                wet_hat, stashes["delay"] = fx.flanger_forward_stash(dry, mod, consts, *geometry, rows=rows, out=wet_hat)
            else:
                wet_hat = fx.flanger_forward(dry, mod, consts, *geometry, rows=rows, out=wet_hat)
        if m["tremolo"].numel():
            wet_hat = fx.tremolo_forward(dry, mod, consts, rows=self._launch_rows(m, "tremolo"), out=wet_hat)
        if m["phaser"].numel():
            wet_hat, st, _ = fx.phaser_forward_stash_lr(dry, consts, None, self.sr, N, mod, rows=self._launch_rows(m, "phaser"),
                                                        out=wet_hat)
            if stash:
                stashes["phaser"] = st
        return wet_hat, stashes

    def _adjoint_rows(self, dy: T, dry: T, mod: T, consts: Dict[str, T], stashes: Dict[str, T],
                      gbuf: Optional[T] = None) -> T:
        """d loss / d LFO (B, n_frames) from d loss / d wet_hat (B, N): every family's adjoint, asked for dmod alone, writes
        its rows of one zero-initialised buffer through the forward's row list (``mx_flanger_bwd_lr``; ``mx_tremolo_bwd``;
        ``mx_phaser_bwd`` + ``mx_phaser_dmod_gather``).  Dry rows keep the zeros.  A family that owns every row writes every
        row: no zeros then, its wrapper's own ``torch.empty``.  ``gbuf`` (6, B) fp64 (a step with ``learned_fx``): every family
        is also asked for the per-clip gradients of the slots its kinds have learned entries for, written into its rows of
        ``gbuf`` (slot order ``fx.FX_SLOTS``); without it nothing but dmod is asked for."""
        from . import fx
        B, N = dry.shape
        m = self._mixed_rows(B, dry.device)
        dmod = None if m["all_rows"] else torch.zeros((B, mod.size(1)), device=dry.device, dtype=torch.float32)

        def wanted(*kinds: str) -> Dict[str, T]:                    # slot name -> its row of gbuf, for the kinds' learned names
            if gbuf is None:
                return {}
            slots = {fx.FX_NAME_SLOT[n] for k in kinds for n in self._fxp.learned(k)}
            return {s: gbuf[i] for i, s in enumerate(fx.FX_SLOTS) if s in slots}

        if m["delay"].numel():
            g = wanted("flanger", "chorus")
            dmod = fx.flanger_backward(dy, dry, mod, stashes["delay"], consts, m["max_delay"], m["max_delay_max"],
                                       rows=self._launch_rows(m, "delay"), need_dx=False,
                                       params=tuple(k for k in fx.PARAM_GRADS if k in g), dmod=dmod, grads=g)[1]
        if m["tremolo"].numel():
            g = wanted("tremolo")
            dmod = fx.tremolo_backward(dy, dry, mod, consts, rows=self._launch_rows(m, "tremolo"), need_dx=False,
                                       need_dmix="mix" in g, dmod=dmod, dmix=g.get("mix"))[1]
        if m["phaser"].numel():
            g = wanted("phaser")
            dmod = fx.phaser_backward_lr(dy, dry, stashes["phaser"], consts, None, self.sr, N, mod.size(1), need_dx=False,
                                         params_wanted=tuple(k for k in fx.PHASER_PARAM_GRADS if k in g),
                                         rows=self._launch_rows(m, "phaser"), dmod=dmod, grads=g)[1]
        return dmod

    @staticmethod
    def _rows(audio: T) -> T:
        assert audio.ndim == 3 and audio.size(1) == 1, "mono clips (B, 1, N)"
        return audio[:, 0, :]

    def render(self, dry: T, mod_sig: T, fx_params, latent: Optional[T] = None) -> T:
        """wet_hat (B, 1, N) = the effect on ``dry`` (B, 1, N) driven by ``mod_sig`` (B, n_mod) at its own rate, with the
        per-clip constants of ``fx_params``; no graph and no stash kept (``_render_rows``: the data path's launches; the
        phaser with lead 0, see the class docstring).  ``latent``: required by a step with ``fx_head`` (a ValueError without
        it), whose forward kernel alone runs then.  There is no ``wet`` here, so the result is NOT gain-matched whatever
        ``match_gain`` says: it is the effect at unit dry gain."""
        rows = self._rows(dry)
        with torch.no_grad():
            consts = self.clip_constants(fx_params, rows.size(0), rows.device, latent)
            y = self._render_rows(rows, mod_sig.detach().float().contiguous(), consts, stash=False)[0]
        return y.unsqueeze(1)

    def audio_loss(self, mod_sig_hat: T, dry: T, wet: T, fx_params, prefix: Optional[str] = None,
                   latent: Optional[T] = None):
        """(loss, wet_hat (B, 1, N)) for an LFO (B, n_frames); with grad mode on and an LFO, ``learned_fx.raw`` or an input of
        ``fx_head`` (``latent``, its weight, its bias) that requires grad the loss carries the graph of ``_EffectAudioLossFn``,
        otherwise nothing is stashed and no backward kernel runs.  ``prefix``: log every audio term under it."""
        from .effect_losses import effect_loss_terms
        dry_r, wet_r = self._rows(dry), self._rows(wet)
        P = self._warmup(dry_r.size(1))                             # its ValueError, before any launch
        terms: Dict[str, T] = {}
        head = self.fx_head
        if head is not None and latent is None:
            raise ValueError("a step with fx_head predicts the effect parameters from the model's latent: pass latent=")
        # the node's differentiable inputs beside the LFO
        params = (latent, head.weight, head.bias) if head is not None else () if self.learned_fx is None else (self.learned_fx.raw,)
        if torch.is_grad_enabled() and any(t.requires_grad for t in (mod_sig_hat, *params)):
            with torch.no_grad():
                consts = self.clip_constants(fx_params, dry_r.size(0), dry_r.device, latent)
            loss, wet_hat = _EffectAudioLossFn.apply(mod_sig_hat, self, dry_r, wet_r, consts, terms, *params)
            wet_hat = wet_hat.unsqueeze(1)
        else:
            wet_hat, loss = self.render(dry, mod_sig_hat, fx_params, latent), None
            if self._matched:                                       # validation: the terms below are taken on the matched rows
                if P:                                               # matched on the window, into [P:] of a (B, 1, N) buffer
                    rendered, wet_hat = wet_hat, torch.empty_like(wet_hat)
                    wet_hat[..., :P] = rendered[..., :P]
                    self._match_rows(rendered[..., P:], wet[..., P:], out=wet_hat[..., P:])
                else:
                    wet_hat = self._match_rows(wet_hat, wet)
                self._shaper_in = None                              # read by a backward only
        if prefix is not None or loss is None:
            with torch.no_grad():
                missing = [k for k in self.audio_loss_dict if k not in terms]
                seen, target = (wet_hat[..., P:], wet[..., P:]) if P else (wet_hat, wet)    # what the losses compare
                if any(k in ("l1", "mse", "esr", "dc") for k in missing):
                    terms.update({k: v for k, v in effect_loss_terms(seen, target).items() if k in missing})
                for k in missing:
                    if k not in terms:
                        terms[k] = self._loss_module(k)(seen, target)
            if loss is None:
                loss = self.weighted_sum(terms, self.audio_loss_dict)
            if prefix is not None:
                for k in self.audio_loss_dict:
                    self.log(f"{prefix}/{k}", terms[k])
        return loss, wet_hat

    def common_step(self, batch, is_training: bool):
        prefix = "train" if is_training else "val"
        dry, wet, mod_sig, fx_params = batch
        assert dry is not None, "the re-render needs the dry clip"
        self._require_fx_params(fx_params, dry.size(0))             # before any launch
        latent = None
        if self.fx_head is None:
            mod_sig_hat, _ = self.model(stack_dry_wet(dry, wet) if self.use_dry else wet)
        else:
            out = self.model(stack_dry_wet(dry, wet) if self.use_dry else wet)
            if not (isinstance(out, (tuple, list)) and len(out) == 2 and isinstance(out[0], T) and isinstance(out[1], T)):
                raise ValueError("fx_head needs a model whose forward returns the pair (lfo, latent), as "
                                 "models.Spectral2DCNN does; this model returns no latent")
            mod_sig_hat, latent = out
            self._head_latent(latent, dry.size(0))                  # its ValueErrors, before any launch
        mod_sig_hat = mod_sig_hat.squeeze(1)
        if mod_sig is not None:
            mod_sig = linear_interpolate_last_dim(mod_sig, mod_sig_hat.size(-1), align_corners=True)
        if self.model_smooth_n_frames > 1:
            n_frames_in = mod_sig_hat.size(-1)
            if mod_sig_hat.requires_grad and torch.is_grad_enabled():
                mod_sig_hat = smoothen_with_grad(mod_sig_hat, self.model_smooth_n_frames)
            else:
                mod_sig_hat = smoothen(mod_sig_hat, self.model_smooth_n_frames)
            n_frames = mod_sig_hat.size(-1)
            if mod_sig is not None:
                mod_sig = self.center_crop_mod_sig(mod_sig, n_frames)
            n_samples = int((n_frames / n_frames_in) * dry.size(-1))            # TBPTTLFOEffectModeling._prepare_all_rows
            dry = self.center_crop_mod_sig(dry, n_samples).contiguous()
            wet = self.center_crop_mod_sig(wet, n_samples).contiguous()
        loss, wet_hat = self.audio_loss(mod_sig_hat, dry, wet, fx_params, prefix, latent)
        if self.lfo_loss_dict and mod_sig is not None:
            lfo_term = self.calc_and_log_losses(mod_sig_hat, mod_sig.contiguous(), self.lfo_loss_dict, f"{prefix}/lfo_",
                                                log_total=False)
            if lfo_term is not None:
                loss = loss + lfo_term
        self.log(f"{prefix}/loss", loss)
        if is_training and self.learned_fx is not None:             # views of the launch's values vector: no host sync
            for i, name in enumerate(self.learned_fx.names):
                self.log(f"fx/{name}", self._fx_values[i])
        if is_training and self.fx_head is not None:                # a handful of (B, P) device operations: no host sync
            m = self._mixed_rows(dry.size(0), dry.device)
            mean = (self._fx_values * m["head_mask"]).sum(0) / m["head_count"]
            std = ((((self._fx_values - mean) ** 2) * m["head_mask"]).sum(0) / m["head_count"]).sqrt()
            for i, name in enumerate(self.fx_head.names):
                self.log(f"fx/{name}", mean[i])
                self.log(f"fx_std/{name}", std[i])
        if is_training and self.match_gain is not None:             # three (B,) device reductions: no host sync
            g = self._gain.gain
            self.log("gain/mean", g.mean())
            self.log("gain/std", g.std(unbiased=False))
            self.log("gain/clamped", self._gain.flags.float().mean())
        if is_training and self.match_fir is not None:              # three (B, K) / (B,) device reductions: no host sync
            h = self._fir.taps
            self.log("fir/dc_gain", h.sum(1).mean())
            self.log("fir/l1", h.abs().sum(1).mean())
            self.log("fir/flagged", (self._fir.flags != 0).float().mean())
        if is_training and self.match_shaper is not None:           # three (B, K) / (B,) device reductions: no host sync
            c = self._shaper.coeffs
            self.log("shaper/linear", c[:, 0].mean())
            self.log("shaper/curve", c[:, 1:].abs().sum(1).mean())
            self.log("shaper/flagged", (self._shaper.flags != 0).float().mean())
        data_dict = {"dry": dry.detach(), "wet": wet.detach(), "wet_hat": wet_hat.detach(),
                     "mod_sig_hat": mod_sig_hat.detach()}
        if self.fx_head is not None:
            data_dict["fx_values"] = self._fx_values
        if self.match_gain is not None:
            data_dict["gain"] = self._gain.gain
        if self.match_fir is not None:
            data_dict["fir"] = self._fir.taps
        if self.match_shaper is not None:
            data_dict["shaper"] = self._shaper.coeffs
        if self.warmup_samples:
            data_dict["warmup"] = self.warmup_samples
        if mod_sig is not None:
            data_dict["mod_sig"] = mod_sig.detach()
        return loss, data_dict, fx_params

    def training_step(self, batch, batch_idx: int = 0) -> T:
        return self.common_step(batch, is_training=True)[0]

    def validation_step(self, batch, batch_idx: int = 0):
        with torch.no_grad():
            return self.common_step(batch, is_training=False)


def _channel_rows(t: T) -> T:
    """(B, C, T) -> (B C, 1, T): the effect-model losses reduce over clips AND channels alike (losses.py:33-38,61-66: a mean over
    (batch, channel) of per-row ratios; nn.L1Loss: a mean over everything)."""
    return t if t.size(1) == 1 else t.contiguous().view(-1, 1, t.size(-1))


class TBPTTLFOEffectModeling(BaseLightingModule):
    """lightning.py:202-431: frozen LFO-net -> smooth / stretch / crop -> discard invalid LFOs -> LSTM
    effect model trained with truncated BPTT (1024-sample warm-up, then one optimizer step per
    1024-sample chunk).  ``automatic_optimization`` is False like in the reference: ``training_step``
    receives the optimizer and runs the 83 inner steps itself; under DDP every inner step is one
    all-reduce of the 70 KB flat gradient, and a rank without any valid LFO still takes part with
    zero gradients (the reference would return None there and dead-lock DDP).

    ``pre_emph_filter_cfs`` / ``pre_emph_low_pass``: the filter of the "esr_pre" loss (``losses.PreEmphESRLoss``; 1 .. 16
    taps).  Every chunk's gradient filters that chunk with its own zero history, which is what ``WrightPreEmph`` does per
    call; the logged ``{prefix}/esr_pre`` is taken over the whole clip after the warm-up, like every other term."""
    default_loss_dict = {"l1": 1.0, "esr": 0.0, "dc": 0.0}

    def __init__(self,
                 warmup_n_samples: int,
                 step_n_samples: int,
                 effect_model: HiddenStateModel,
                 lfo_model: Optional[nn.Module] = None,
                 lfo_model_weights_path: Optional[str] = None,
                 freeze_lfo_model: bool = True,
                 param_model: Optional[nn.Module] = None,
                 sr: float = 44100,
                 use_dry: bool = True,
                 model_smooth_n_frames: int = 8,
                 should_stretch: bool = True,
                 max_n_corners: int = 16,
                 stretch_smooth_n_frames: int = 0,
                 discard_invalid_lfos: bool = True,
                 loss_dict: Optional[Dict[str, float]] = None,
                 pre_emph_filter_cfs: Sequence[float] = (-0.95, 1.0),
                 pre_emph_low_pass: bool = False) -> None:
        super().__init__(loss_dict)
        self._set_pre_emph(pre_emph_filter_cfs, pre_emph_low_pass)
        assert warmup_n_samples > 0
        # param_model (lightning.py:344-347,371-375): any nn.Module wet (B, C, n) -> (B, P); its output is repeated over time and
        # concatenated to the LFO as extra latent channels (the effect model then has latent_dim = 1 + P, i.e. the general LSTM
        # of lstm_generic.py, an autograd node -- the step below runs such models through `_general_train_chunk`).
        # freeze_lfo_model: false (lightning.py:258,344-366): the extractor is re-run inside every TBPTT step and trained through the
        # effect model -- CNN -> moving average -> stretch_corners -> resampling -> LSTM, every stage with a backward kernel
        # (common_step below, `relearn`).
        from .effect_losses import GRAD_NAMES
        for name, w in self.loss_dict.items():
            if w > 0 and name not in GRAD_NAMES:
                raise NotImplementedError(f"effect-model loss '{name}' has no gradient kernel (supported: {GRAD_NAMES})")
        # only nn.L1Loss weighted (every shipped config): the BPTT kernel evaluates its gradient itself
        self._fused_l1 = all(w <= 0 or name == "l1" for name, w in self.loss_dict.items())
        self.warmup_n_samples, self.step_n_samples = warmup_n_samples, step_n_samples
        self.effect_model = effect_model
        self.lfo_model_weights_path = lfo_model_weights_path
        self.freeze_lfo_model = freeze_lfo_model
        self.param_model = param_model
        self.sr, self.use_dry = sr, use_dry
        self.model_smooth_n_frames = model_smooth_n_frames
        self.should_stretch, self.max_n_corners = should_stretch, max_n_corners
        self.stretch_smooth_n_frames = stretch_smooth_n_frames
        self.discard_invalid_lfos = discard_invalid_lfos
        if lfo_model is not None:
            if lfo_model_weights_path is not None:
                log.info("Loading LFO model weights")
                assert os.path.isfile(lfo_model_weights_path)
                lfo_model.load_state_dict(torch.load(lfo_model_weights_path, map_location="cpu"))
            if freeze_lfo_model:
                log.info("Freezing LFO model")
                lfo_model.eval()
                for p in lfo_model.parameters():
                    p.requires_grad = False
        else:
            log.info("Using ground truth mod_sig")
        self.lfo_model = lfo_model
        self.automatic_optimization = False
        self.use_gt_mod_sig = lfo_model is None

    def train(self, mode: bool = True):
        super().train(mode)
        if self.lfo_model is not None and self.freeze_lfo_model:
            self.lfo_model.eval()               # frozen extractor stays in eval mode (lightning.py:243-244)
        return self

    def extract_mod_sig(self, wet: T, mod_sig: Optional[T] = None, fx_params=None):
        """lightning.py:254-272."""
        with torch.no_grad():
            if self.lfo_model is None:
                assert mod_sig is not None and mod_sig.ndim == 2
                mod_sig_hat = mod_sig
            elif isinstance(self.lfo_model, RandomLFO):
                mod_sig_hat = self.lfo_model(wet.size(0), fx_params).squeeze(1).to(wet.device)
            else:
                mod_sig_hat, _ = self.lfo_model(wet)
                mod_sig_hat = mod_sig_hat.squeeze(1)
            if mod_sig is not None and mod_sig.size(-1) != mod_sig_hat.size(-1):
                mod_sig = linear_interpolate_last_dim(mod_sig, mod_sig_hat.size(-1), align_corners=True)
            return mod_sig_hat, mod_sig

    def smooth_stretch_crop_mod_sig(self, mod_sig_hat: T, mod_sig: Optional[T] = None):
        """lightning.py:284-300."""
        orig = mod_sig_hat.size(-1)
        if self.model_smooth_n_frames > 1:
            mod_sig_hat = smoothen(mod_sig_hat, self.model_smooth_n_frames)
            if mod_sig is not None:
                mod_sig = self.center_crop_mod_sig(mod_sig, mod_sig_hat.size(-1))
        if self.should_stretch:
            mod_sig_hat = stretch_corners(mod_sig_hat, max_n_corners=self.max_n_corners,
                                          smooth_n_frames=self.stretch_smooth_n_frames)
            if self.stretch_smooth_n_frames > 1 and mod_sig is not None:
                mod_sig = self.center_crop_mod_sig(mod_sig, mod_sig_hat.size(-1))
        return mod_sig_hat, mod_sig, orig - mod_sig_hat.size(-1)

    def _prepare_all_rows(self, batch):
        """lightning.py:310-326 for EVERY clip of the batch, without a host synchronisation: extractor forward, smooth /
        stretch / crop, and the validity verdict of each row as a device tensor (None when nothing is discarded)."""
        dry, wet, mod_sig, fx_params = batch
        assert dry.size(-1) == wet.size(-1) >= self.warmup_n_samples + self.step_n_samples
        lfo_in = stack_dry_wet(dry, wet) if self.use_dry else wet
        mod_sig_hat, mod_sig = self.extract_mod_sig(lfo_in, mod_sig, fx_params)
        mod_sig_hat, mod_sig, removed = self.smooth_stretch_crop_mod_sig(mod_sig_hat, mod_sig)
        n_frames = mod_sig_hat.size(-1)
        n_samples = int((n_frames / (n_frames + removed)) * dry.size(-1))
        dry = self.center_crop_mod_sig(dry, n_samples)
        wet = self.center_crop_mod_sig(wet, n_samples)
        valid = valid_mod_sig_mask(mod_sig_hat) if self.discard_invalid_lfos else None
        return dry, wet, mod_sig_hat, mod_sig, valid

    def _select_rows(self, dry, wet, mod_sig_hat, mod_sig, keep):
        """lightning.py:327-337: drop the clips without a valid LFO (``keep``: host index tensor or None = all rows)
        and resample the LFOs to the audio rate."""
        self.last_kept = dry.size(0) if keep is None else int(keep.numel())      # clips that train this batch
        if keep is not None and keep.numel() == 0:
            log.info("No valid LFO signals found")
            return None
        if keep is not None and keep.numel() < dry.size(0):
            # (pinned: a copy from pageable memory holds the HOST until the stream has reached it, i.e. until the whole
            #  previous batch has run -- and the device then idles while the host catches up)
            if dry.is_cuda:
                keep = keep.pin_memory()
            keep = keep.to(dry.device, non_blocking=True)
            dry, wet, mod_sig_hat = dry[keep], wet[keep], mod_sig_hat[keep]
            if mod_sig is not None:
                mod_sig = mod_sig[keep]
        dry, wet = dry.contiguous(), wet.contiguous()
        lfo_sr = linear_interpolate_last_dim(mod_sig_hat, dry.size(-1), align_corners=True).unsqueeze(1)
        return dry, wet, mod_sig_hat, mod_sig, lfo_sr

    def prepare(self, batch):
        """lightning.py:310-337: everything before the LSTM loop.  Returns None if no clip has a valid
        LFO, else (dry, wet, mod_sig_hat, mod_sig, lfo_at_sample_rate (B',1,n'))."""
        dry, wet, mod_sig_hat, mod_sig, valid = self._prepare_all_rows(batch)
        keep = None if valid is None else torch.nonzero(valid.cpu()).view(-1)
        return self._select_rows(dry, wet, mod_sig_hat, mod_sig, keep)

    def prepare_ahead(self, batch):
        """``prepare`` for a data module's ``set_ahead_fn``: everything before the LSTM loop depends only on the batch
        and on the FROZEN extractor, so it can run one batch ahead on the side stream (the reference gets the same
        overlap from its DataLoader workers for the rendering; the extractor forward is prefetched on top).
        It must not block the host -- the caller still has the 83 optimizer steps of the CURRENT batch to enqueue -- so
        the row verdicts of ``discard_invalid_lfos`` travel to pinned host memory asynchronously behind an event, and
        the gather of the surviving rows happens in ``finish_prepare`` when the batch is consumed."""
        dry, wet, mod_sig_hat, mod_sig, valid = self._prepare_all_rows(batch)
        prep = {"dry": dry, "wet": wet, "mod_sig_hat": mod_sig_hat, "mod_sig": mod_sig, "valid_host": None, "ready": None}
        if valid is not None:
            host = torch.empty(valid.shape, dtype=valid.dtype, pin_memory=True)
            host.copy_(valid, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(valid.device))
            prep["valid_host"], prep["ready"], prep["valid"] = host, ev, valid
        return prep

    def finish_prepare(self, prep):
        """Second half of a prefetched ``prepare``: wait for the (long finished) verdict copy, gather the valid rows on
        the consuming stream.  Returns what ``prepare`` returns."""
        keep = None
        if prep["valid_host"] is not None:
            prep["ready"].synchronize()
            keep = torch.nonzero(prep["valid_host"]).view(-1)
        return self._select_rows(prep["dry"], prep["wet"], prep["mod_sig_hat"], prep["mod_sig"], keep)

    def common_step(self, batch, is_training: bool, optimizer=None, world_size: int = 1, prep=None):
        """lightning.py:302-419."""
        from .effect_losses import effect_loss_grad, effect_loss_terms
        from .trainer import allreduce_flat_grad
        prefix = "train" if is_training else "val"
        prep = self.prepare(batch) if prep is None else self.finish_prepare(prep)
        n_chunks_max = (batch[0].size(-1) - self.warmup_n_samples) // self.step_n_samples
        if prep is None:
            if is_training and world_size > 1:          # stay in lock-step with the other ranks
                self._idle_steps(optimizer, world_size, n_chunks_max)
            return None
        dry, wet, mod_sig_hat, mod_sig, lfo_sr = prep
        em, W, S = self.effect_model, self.warmup_n_samples, self.step_n_samples
        n = dry.size(-1)
        B = dry.size(0)
        # lightning.py:344-349: an UNFROZEN extractor is re-run inside every training step (on the full-length, unfiltered
        # input -- the reference does not re-apply its validity filter there, so it only works when no clip was dropped)
        relearn = (is_training and self.lfo_model is not None and not self.freeze_lfo_model
                   and not isinstance(self.lfo_model, RandomLFO))
        # effect models outside the fused LSTM-64 kernels, and every step with a param_model, go through autograd
        general = bool(getattr(em, "generic", False)) or self.param_model is not None
        lfo_in = None
        if relearn:
            if B != batch[0].size(0):
                raise ValueError("freeze_lfo_model: false re-extracts the LFO of EVERY clip inside the step (lightning.py:344-349): "
                                 "it cannot be combined with clips dropped by discard_invalid_lfos")
            lfo_in = stack_dry_wet(batch[0], batch[1]) if self.use_dry else batch[1]
        from .models import LSTM_NPARAM
        if relearn and not general:
            g_off = (em.lstm.weight_ih_l0.grad.data_ptr() - optimizer.flat_grad.data_ptr()) // 4
            assert em.fc.bias.grad.data_ptr() == optimizer.flat_grad.data_ptr() + 4 * (g_off + LSTM_NPARAM - 1), \
                "the effect model's parameters must be contiguous in the flat gradient (state-dict order)"
            lstm_grad = optimizer.flat_grad[g_off:g_off + LSTM_NPARAM]
        em.clear_hidden()
        with torch.no_grad():
            param_latent = None
            if general:
                if self.param_model is not None:
                    param_latent = self.param_model(wet).unsqueeze(-1)            # lightning.py:344-347
                chunks = [em(dry[:, :, :W], self._with_params(lfo_sr[:, :, :W], param_latent))]
            else:
                chunks = [em.run_chunk(dry[:, :, :W], lfo_sr[:, :, :W])[0]]          # warm-up, no loss
            if is_training:
                em.detach_hidden()
            if is_training and not general:
                stash = torch.empty((B, S, 384), device=dry.device, dtype=torch.float32)
                w_l1 = float(self.loss_dict.get("l1", 0.0))
            done = 0
            for start in range(W, n, S):
                end = start + S
                if end > n:
                    break
                x, lat, tgt = dry[:, :, start:end], lfo_sr[:, :, start:end], wet[:, :, start:end]
                if general and is_training:
                    y, lfo_sr, mod_sig_hat = self._general_train_chunk(x, tgt, wet, lfo_sr, mod_sig_hat, start, end, lfo_in if relearn
                                                                       else None, optimizer, world_size)
                    done += 1
                elif general:
                    y = em(x, self._with_params(lat, param_latent))
                elif relearn:
                    # lightning.py:344-384 with the extractor in the graph: CNN -> moving average -> resampling -> this chunk
                    # of the LFO -> LSTM -> loss; backward in the opposite order, every stage on its own kernel
                    optimizer.zero_grad()
                    hat, hs, hst, lfo_sr = self._extract_in_graph(lfo_in, n)
                    lat = lfo_sr[:, :, start:end]
                    y, h0, c0 = em.run_chunk(x, lat, stash)
                    if self._fused_l1:
                        dlat = em.bptt_chunk_dlfo(x, lat, y, stash, h0, c0, lstm_grad, wet=tgt, loss_scale=w_l1 / (B * S))
                    else:
                        dy = effect_loss_grad(y, tgt, self.loss_dict, **self._grad_modules())
                        dlat = em.bptt_chunk_dlfo(x, lat, y, stash, h0, c0, lstm_grad, dy=dy)
                    self._extract_backward(hat, hs, hst, dlat[:, 0, :], n, start)
                    optimizer.step(grad_scale=allreduce_flat_grad(optimizer.flat_grad, world_size))
                    em.detach_hidden()
                    mod_sig_hat = hst
                    done += 1
                elif is_training:
                    y, h0, c0 = em.run_chunk(x, lat, stash)
                    # no zero_grad(): the BPTT launch OVERWRITES the whole flat gradient (one fill kernel less per step)
                    if self._fused_l1 and world_size == 1 and optimizer.numel == LSTM_NPARAM:
                        # one process, only the LSTM trained: row sum + AdamW in one launch (bit-identical to the two below)
                        optimizer.step_from_rows(em.bptt_l1_chunk(x, lat, y, tgt, stash, h0, c0, w_l1 / (B * S), None))
                        em.detach_hidden()
                        done += 1
                        chunks.append(y)
                        continue
                    if self._fused_l1:
                        em.bptt_l1_chunk(x, lat, y, tgt, stash, h0, c0, w_l1 / (B * S), optimizer.flat_grad)
                    else:       # lightning.py:380-382 with any loss_dict: d loss / d y from the loss kernels, then BPTT
                        dy = effect_loss_grad(y, tgt, self.loss_dict, **self._grad_modules())
                        em.bptt_chunk(x, lat, y, dy, stash, h0, c0, optimizer.flat_grad)
                    optimizer.step(grad_scale=allreduce_flat_grad(optimizer.flat_grad, world_size))
                    em.detach_hidden()
                    done += 1
                else:
                    y = em.run_chunk(x, lat)[0]
                chunks.append(y)
            if is_training and world_size > 1:          # ranks may have cropped differently: pad the step count
                self._idle_steps(optimizer, world_size, n_chunks_max - done)
            wet_hat = torch.cat(chunks, dim=-1)
            m = wet_hat.size(-1)
            dry_c, wet_c, wet_hat = dry[:, :, W:m], wet[:, :, W:m].contiguous(), wet_hat[:, :, W:m].contiguous()
            wet_c = wet_c.expand_as(wet_hat).contiguous() if wet_c.shape != wet_hat.shape else wet_c
            terms = effect_loss_terms(_channel_rows(wet_hat), _channel_rows(wet_c))
            for name in self.loss_dict:
                if name not in terms:
                    terms[name] = self._loss_module(name)(_channel_rows(wet_hat), _channel_rows(wet_c))
            for name in self.loss_dict:
                self.log(f"{prefix}/{name}", terms[name])
            loss = self.weighted_sum(terms, self.loss_dict)
            self.log(f"{prefix}/loss", loss)
        data_dict = {"dry": dry_c, "wet": wet_c, "wet_hat": wet_hat, "mod_sig_hat": mod_sig_hat}
        if mod_sig is not None:
            data_dict["mod_sig"] = mod_sig
        return loss, data_dict, batch[3]

    @staticmethod
    def _with_params(lfo: T, param_latent: Optional[T]) -> T:
        """lightning.py:345-347,374-375: the param_model's vector repeated over the chunk, after the LFO channel."""
        if param_latent is None:
            return lfo
        return torch.cat([lfo, param_latent.repeat(1, 1, lfo.size(-1))], dim=1)

    @staticmethod
    def _idle_steps(optimizer, world_size: int, count: int) -> None:
        """``count`` optimizer steps on an all-reduced zero gradient: a rank with fewer chunks than the others (or none) stays
        in lock-step with them."""
        from .trainer import allreduce_flat_grad
        for _ in range(count):
            optimizer.zero_grad()
            optimizer.step(grad_scale=allreduce_flat_grad(optimizer.flat_grad, world_size))

    def _extract_in_graph(self, lfo_in: T, n: int):
        """The UNFROZEN extractor's forward chain (lightning.py:344-366): CNN (the only stage that records a graph) -> moving
        average -> stretch_corners -> resampling to ``n`` samples.  Returns (hat, hs, hst, the audio-rate LFO (B, 1, n))."""
        with torch.enable_grad():
            hat, _ = self.lfo_model(lfo_in)
        hs = smoothen(hat.detach().squeeze(1), self.model_smooth_n_frames)
        hst = stretch_corners(hs, max_n_corners=self.max_n_corners, smooth_n_frames=self.stretch_smooth_n_frames) \
            if self.should_stretch else hs
        return hat, hs, hst, linear_interpolate_last_dim(hst, n, align_corners=True).unsqueeze(1)

    def _extract_backward(self, hat: T, hs: T, hst: T, d_lfo: T, n: int, start: int) -> None:
        """The backward of ``_extract_in_graph`` from d loss / d LFO (B, chunk) of the chunk at ``start``, every stage on its own
        kernel: resampling window -> stretch_corners -> moving average -> ``hat.backward``."""
        d_hs = linear_interpolate_last_dim_bwd(d_lfo, hst.size(-1), n, start)
        if self.should_stretch:
            d_hs = stretch_corners_bwd(hs, d_hs, max_n_corners=self.max_n_corners, smooth_n_frames=self.stretch_smooth_n_frames)
        d_hs = smoothen_bwd(d_hs, self.model_smooth_n_frames)       # transpose of the moving average
        hat.backward(d_hs.view_as(hat))

    def _general_train_chunk(self, x, tgt, wet, lfo_sr, mod_sig_hat, start, end, lfo_in, optimizer, world_size):
        """One TBPTT training step (lightning.py:358-384) with the effect model as an autograd node: any LSTM size, a
        param_model in the graph (re-evaluated on every step like the reference does), and -- ``lfo_in`` given -- the unfrozen
        extractor re-run and trained through the LFO it produces (the backward chain of the fused path: resampling window ->
        stretch_corners -> moving average -> CNN)."""
        from .effect_losses import effect_loss_grad
        from .trainer import allreduce_flat_grad
        em, n = self.effect_model, wet.size(-1)
        optimizer.zero_grad()
        with torch.enable_grad():
            hat = None
            if lfo_in is not None:
                hat, hs, hst, lfo_sr = self._extract_in_graph(lfo_in, n)
                mod_sig_hat = hst
            lat_lfo = lfo_sr[:, :, start:end]
            if hat is not None:
                lat_lfo = lat_lfo.detach().clone().requires_grad_(True)
            p = self.param_model(wet).unsqueeze(-1) if self.param_model is not None else None       # lightning.py:371-373
            y = em(x, self._with_params(lat_lfo, p))
        tgt = tgt.expand_as(y) if tgt.shape != y.shape else tgt
        dy = effect_loss_grad(_channel_rows(y.detach()), _channel_rows(tgt), self.loss_dict, **self._grad_modules())
        y.backward(dy.view_as(y))
        if hat is not None:
            self._extract_backward(hat, hs, hst, lat_lfo.grad[:, 0, :].contiguous(), n, start)
        optimizer.step(grad_scale=allreduce_flat_grad(optimizer.flat_grad, world_size))
        em.detach_hidden()
        return y.detach(), lfo_sr, mod_sig_hat

    def training_step(self, batch, batch_idx: int = 0, optimizer=None, world_size: int = 1, prep=None):
        assert optimizer is not None, "manual optimisation: pass the FlatAdamW optimizer"
        result = self.common_step(batch, is_training=True, optimizer=optimizer, world_size=world_size, prep=prep)
        return None if result is None else result[0]

    def validation_step(self, batch, batch_idx: int = 0):
        return self.common_step(batch, is_training=False)

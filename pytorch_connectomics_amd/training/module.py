"""Lightning-free counterpart of the reference's ConnectomicsModule (training/lightning/model.py:74-1256) for
the hot path: forward / training_step / validation_step / configure_optimizers with the same method names,
a two-term loss (weighted BCE-with-logits + sigmoid Dice, profiles/loss_profiles.yaml:2-9) with deep-supervision
weights [1, .5, .25, .125, .0625] (schema/model.py:46-51), AdamW with the no-weight-decay-on-norm grouping
(training/optimization/build.py:73-112), WarmupCosineLR (lr_scheduler.py:48-82), global-norm gradient clipping,
DDP over RCCL, and Lightning-layout checkpoints ("state_dict" with the "model." prefix, model.py:244-297).

The network forward/backward run the HIP kernels; on a GPU the BCE + Dice loss and the clip + AdamW (+ EMA) update
are HIP kernels too (training/fused.py); other loss functions and optimizers are PyTorch
device ops.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Mapping, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..models import build_model
from ..utils.channel_slices import resolve_channel_indices, resolve_channel_range
from ..utils.model_outputs import _cfg_value as _cfg_get
from ..utils.model_outputs import resolve_configured_output_head, resolve_head_target_slice, select_output_tensor, unwrap_main_output
from .loss_table import loss_row
from .metrics import ConfusionState, metrics_from_counts
from .losses import (_mask_for_unweighted_loss, auto_pos_weight_scalar, class_balance_weight,  # noqa: F401  (re-exported: callers
                     dice_loss_sigmoid, monai_dice_loss, monai_focal_loss, monai_tversky_loss,     # and the exact-epilogue tests read
                     per_channel_bce_with_logits, weighted_bce_with_logits, weighted_regression_loss)   # them from this module)

_NORM_TYPES = (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d, nn.SyncBatchNorm, nn.GroupNorm, nn.InstanceNorm1d,
               nn.InstanceNorm2d, nn.InstanceNorm3d, nn.LayerNorm, nn.LocalResponseNorm)
DS_WEIGHTS = [1.0, 0.5, 0.25, 0.125, 0.0625]


def match_target_to_output(target: torch.Tensor, output: torch.Tensor) -> torch.Tensor:
    """Deep-supervision target at an output's resolution (training/losses/orchestrator.py:892-952): integer labels by nearest
    neighbour (kept integer), dense float targets by trilinear interpolation (align_corners=False) and clamped back to
    [-1, 1] / [0, 1] when the original lies in that range (interpolation overshoot of tanh-SDT / sigmoid targets)."""
    if target.shape == output.shape:
        return target
    if target.dtype in (torch.long, torch.int, torch.int32, torch.int64, torch.uint8):
        return F.interpolate(target.float(), size=output.shape[2:], mode="nearest").long()
    # (B, C, H, W) targets of a dim='2d' model: the bilinear twin (the reference names "trilinear" unconditionally, which
    # torch rejects for 4-D tensors, so its 2-D + deep-supervision configs cannot reach this line)
    out = F.interpolate(target, size=output.shape[2:], mode="trilinear" if target.dim() == 5 else "bilinear", align_corners=False)
    lo, hi = float(target.min()), float(target.max())
    if lo >= -1.5 and hi <= 1.5:
        out = torch.clamp(out, -1.0, 1.0)
    elif lo >= 0.0 and hi <= 1.5:
        out = torch.clamp(out, 0.0, 1.0)
    return out


def resize_class_index_to_output(t: torch.Tensor, output: torch.Tensor) -> torch.Tensor:
    """Nearest-neighbour resize regardless of dtype (orchestrator.py:277-291): batch masks and class-index targets."""
    if t.shape[2:] == output.shape[2:]:
        return t
    r = F.interpolate(t.float(), size=output.shape[2:], mode="nearest")
    return r.to(t.dtype) if t.dtype.is_floating_point else r.long()


def check_label_mask(label_mask: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """The per-channel valid mask the label transform emits, as the float factor the loss terms multiply (orchestrator.py:484-498):
    bool, or the device transform's fp32 0 / 1 form, of the labels' shape."""
    if label_mask.dtype not in (torch.bool, torch.float32):
        raise TypeError(f"label_mask must have dtype torch.bool, got {label_mask.dtype}")
    if label_mask.shape[:2] != labels.shape[:2] or label_mask.shape[2:] != labels.shape[2:]:
        raise ValueError("label_mask must have the same batch, channel, and spatial shape as labels: "
                         f"label_mask={tuple(label_mask.shape)}, labels={tuple(labels.shape)}")
    return label_mask if label_mask.dtype == torch.float32 else label_mask.to(torch.float32)


def resize_label_mask_to_output(label_mask: torch.Tensor, output: torch.Tensor) -> torch.Tensor:
    """A (float 0 / 1) label mask at a deep-supervision output's resolution (orchestrator.py:405-422): the invalid voxels are
    area-averaged, and a coarse voxel is valid only if no fine voxel under it is invalid."""
    if label_mask.shape[2:] == output.shape[2:]:
        return label_mask
    invalid = F.interpolate(1.0 - label_mask, size=output.shape[2:], mode="area")
    return (invalid <= 0.0).to(label_mask.dtype)


class WarmupCosineLR(torch.optim.lr_scheduler.LRScheduler):
    """lr = eta_min + (base * warmup(t) - eta_min) * 0.5 (1 + cos(pi t / max_iters))."""

    def __init__(self, optimizer, max_iters: int, warmup_factor: float = 0.001, warmup_iters: int = 1000,
                 eta_min: float = 0.0, last_epoch: int = -1):
        self.max_iters, self.warmup_factor, self.warmup_iters, self.eta_min = max_iters, warmup_factor, warmup_iters, eta_min
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        it = self.last_epoch
        wf = 1.0
        if it < self.warmup_iters:
            alpha = it / max(1, self.warmup_iters)
            wf = self.warmup_factor * (1 - alpha) + alpha
        cos = 0.5 * (1.0 + math.cos(math.pi * it / self.max_iters))
        return [self.eta_min + (b * wf - self.eta_min) * cos for b in self.base_lrs]


def build_optimizer(cfg, model: nn.Module) -> torch.optim.Optimizer:
    oc = cfg.optimization.optimizer
    name = str(getattr(oc, "name", "adamw")).lower()
    lr = float(getattr(oc, "lr", 1e-4))
    wd = float(getattr(oc, "weight_decay", 1e-4))
    wd_norm = float(getattr(oc, "weight_decay_norm", 0.0))
    wd_bias = float(getattr(oc, "weight_decay_bias", wd))
    bias_lr = float(getattr(oc, "bias_lr_factor", 1.0))
    # the reference (optimization/build.py:73-112) emits one group per parameter; parameters with identical
    # hyper-parameters are merged here (same update rule, but the multi-tensor optimizer then runs a handful of fused
    # launches per step instead of ~8 per parameter -- 1 800 tiny launches / 40 ms of host time for MedNeXt-S)
    merged, seen, seen_order = {}, set(), []
    for module in model.modules():
        for key, p in module.named_parameters(recurse=False):
            if not p.requires_grad or p in seen:
                continue
            seen.add(p)
            seen_order.append(p)
            g_lr, g_wd = lr, wd
            if isinstance(module, _NORM_TYPES):
                g_wd = wd_norm
            elif key == "bias":
                g_lr, g_wd = lr * bias_lr, wd_bias
            merged.setdefault((g_lr, g_wd), []).append(p)
    groups = [{"params": ps, "lr": k[0], "weight_decay": k[1]} for k, ps in merged.items()]
    model_order = {id(p): i for i, p in enumerate(p for p in seen_order)}
    betas = tuple(getattr(oc, "betas", (0.9, 0.999)))
    eps = float(getattr(oc, "eps", 1e-8))
    if name == "adamw":
        fused = bool(getattr(oc, "fused", True)) and all(p.is_cuda for g in groups for p in g["params"])
        if fused:
            # one multi-tensor HIP launch for the clip norm and one for the update (training/fused.py); the clip value
            # of optimization.gradient_clip_val is applied inside, so fit() skips torch's clip_grad_norm_
            from .fused import FusedAdamW
            ema = getattr(cfg.optimization, "ema", None)
            ema_on = bool(getattr(ema, "enabled", False)) if ema is not None else False
            opt = FusedAdamW(groups, lr=lr, betas=betas, eps=eps, weight_decay=wd,
                             max_grad_norm=float(getattr(cfg.optimization, "gradient_clip_val", 0.0) or 0.0),
                             ema_decay=float(getattr(ema, "decay", 0.999)) if ema_on else None,
                             ema_warmup_steps=int(getattr(ema, "warmup_steps", 0) or 0) if ema_on else 0)
        else:
            opt = torch.optim.AdamW(groups, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    elif name == "adam":
        opt = torch.optim.Adam(groups, lr=lr, betas=betas, eps=eps)
    elif name == "sgd":
        opt = torch.optim.SGD(groups, lr=lr, momentum=float(getattr(oc, "momentum", 0.9)), weight_decay=wd,
                              nesterov=bool(getattr(oc, "nesterov", False)))
    else:
        raise ValueError(f"Unknown optimizer: '{name}'. Supported optimizers: adamw, adam, sgd")
    opt._pytc_model_order = model_order          # position of every parameter in registration order (checkpoint remapping)
    return opt


def _sched_param(sc, key, default, *, specific=False):
    """optimization/build.py:30-44: `scheduler.params[key]` first; then (unless scheduler-specific) the direct field."""
    params = getattr(sc, "params", None)
    if isinstance(params, Mapping) and key in params and params[key] is not None:
        return params[key]
    if specific:
        return default
    v = getattr(sc, key, default)
    return default if v is None else v


def build_lr_scheduler(cfg, optimizer):
    """The reference's scheduler table (optimization/build.py:155-324): cosineannealinglr (default, also for unknown names),
    cosineannealingwarmrestarts, steplr, multisteplr, reducelronplateau, warmupcosine[lr], constant[lr]; parameters from
    `scheduler.params` then the typed fields; `name: null` = no scheduler.  WarmupCosineLR also accepts the round-1 spellings
    (max_iters / warmup_iters / warmup_factor)."""
    from torch.optim import lr_scheduler as LS
    sc = getattr(cfg.optimization, "scheduler", None)
    if sc is None or getattr(sc, "name", "cosineannealinglr") is None:
        return None
    name = str(_sched_param(sc, "name", "cosineannealinglr")).lower()
    max_epochs = int(getattr(cfg.optimization, "max_epochs", 100) or 100)
    if name in ("cosineannealingwarmrestarts", "cosinewarmrestarts"):
        return LS.CosineAnnealingWarmRestarts(optimizer, T_0=int(_sched_param(sc, "T_0", 200, specific=True)),
                                              T_mult=int(_sched_param(sc, "T_mult", 1, specific=True)),
                                              eta_min=float(_sched_param(sc, "min_lr", 1e-5)))
    if name == "steplr":
        return LS.StepLR(optimizer, step_size=int(_sched_param(sc, "step_size", 30, specific=True)),
                         gamma=float(_sched_param(sc, "gamma", 0.1, specific=True)))
    if name == "multisteplr":
        return LS.MultiStepLR(optimizer, milestones=list(_sched_param(sc, "milestones", [30, 60, 90], specific=True)),
                              gamma=float(_sched_param(sc, "gamma", 0.1, specific=True)))
    if name == "reducelronplateau":
        return LS.ReduceLROnPlateau(optimizer, mode=_sched_param(sc, "mode", "min"), factor=float(_sched_param(sc, "factor", 0.1)),
                                    patience=int(_sched_param(sc, "patience", 10)), threshold=float(_sched_param(sc, "threshold", 1e-4)),
                                    cooldown=int(_sched_param(sc, "cooldown", 0)), eps=float(_sched_param(sc, "eps", 1e-8)),
                                    min_lr=float(_sched_param(sc, "min_lr", 1e-6)))
    if name in ("warmupcosine", "warmupcosinelr", "warmup_cosine", "warmup_cosine_lr"):
        max_iter = _sched_param(sc, "max_iter", None, specific=True) or getattr(sc, "max_iters", None) or max_epochs
        warm = getattr(sc, "warmup_iters", None)
        factor = getattr(sc, "warmup_factor", None)
        return WarmupCosineLR(optimizer, int(max_iter),
                              warmup_factor=float(factor if factor is not None else _sched_param(sc, "warmup_start_lr", 0.001)),
                              warmup_iters=int(warm if warm is not None else _sched_param(sc, "warmup_epochs", 5)),
                              eta_min=float(_sched_param(sc, "min_lr", 0.0)))
    if name in ("constant", "constantlr"):
        return LS.LambdaLR(optimizer, lr_lambda=lambda epoch: 1.0)
    if name != "cosineannealinglr":
        import logging
        logging.getLogger(__name__).warning("unknown scheduler %r: using CosineAnnealingLR like the reference builder", name)
    return LS.CosineAnnealingLR(optimizer, T_max=int(_sched_param(sc, "t_max", max_epochs, specific=True)),
                                eta_min=float(_sched_param(sc, "min_lr", 1e-6)))


_DEFAULT_TERMS = [{"function": "WeightedBCEWithLogitsLoss", "weight": 1.0},
                  {"function": "DiceLoss", "weight": 1.0, "kwargs": {"sigmoid": True}}]


def plan_loss_terms(cfg) -> list:
    """model.loss.losses -> the term mappings `_term_loss` works from (training/losses/plan.py:126-237), every check of a term run
    here, when the module is built.  A term's loss is built once (`loss`), from its row of training/loss_table.py (`row`)."""
    terms = getattr(getattr(cfg.model, "loss", None), "losses", None) or _DEFAULT_TERMS
    heads = getattr(cfg.model, "heads", None)
    heads = heads if isinstance(heads, Mapping) else {}
    primary = getattr(cfg.model, "primary_head", None)
    plan = []
    for n, t in enumerate(terms):
        get = t.get if isinstance(t, dict) else (lambda k, d=None, _t=t: getattr(_t, k, d))
        where = f"losses[{n}]"
        fn, kwargs = get("function"), dict(get("kwargs", None) or {})
        row = loss_row(fn, kwargs)
        loss = row.build(**kwargs)                 # the loss's argument checks run when the module is built, as in the reference
        # how the loss is called (training/losses/plan.py:158-237): the kind is the loss's own; a term may restate it
        call_kind = str(get("call_kind", get("call", row.call)))
        if call_kind != row.call:
            raise ValueError(f"Unsupported call_kind {call_kind!r} in {where}")
        pos_weight = get("pos_weight")
        if isinstance(pos_weight, str):
            if pos_weight.strip().lower() != "auto":
                raise ValueError(f"{where} pos_weight must be a positive number or 'auto', got {pos_weight!r}")
            pos_weight = "auto"
        elif pos_weight is not None and float(pos_weight) <= 0:
            raise ValueError(f"{where} pos_weight must be > 0, got {float(pos_weight)}")
        # which head a term reads is settled when the module is built (training/losses/plan.py:183-229): pred_head, else
        # model.primary_head, else the only head; a term that names no target channels takes that head's `target_slice`
        pred_head, pred2_head = get("pred_head"), get("pred2_head")
        if heads:
            if pred_head is not None and pred_head not in heads:
                raise ValueError(f"{where} pred_head={pred_head!r} is not one of the configured model.heads {sorted(heads)}")
            if pred2_head is not None and pred2_head not in heads:
                raise ValueError(f"{where} pred2_head={pred2_head!r} is not one of the configured model.heads {sorted(heads)}")
            if pred_head is None and primary is None and len(heads) > 1:
                raise ValueError(f"{where} must define pred_head or model.primary_head when model.heads has multiple entries "
                                 f"{sorted(heads)}")
        elif pred_head is not None or pred2_head is not None:
            raise ValueError(f"{where} uses pred_head/pred2_head but model.heads is not configured.")
        pred_slice, pred2_slice = get("pred_slice", get("pred")), get("pred2_slice", get("pred2"))
        if call_kind == "pred_only" and pred_slice is None:
            raise ValueError(f"{where} pred_only terms require pred_slice")
        if call_kind == "pred_pred" and (pred_slice is None or pred2_slice is None):
            raise ValueError(f"{where} pred_pred terms require pred_slice and pred2_slice")
        if pos_weight is not None and row.spatial != "weight":
            raise ValueError(f"{where} pos_weight is only supported for losses with "
                             f"spatial_weight_arg='weight' (got {fn})")
        target_slice = get("target_slice", get("target"))
        if target_slice is None and call_kind == "pred_target":
            head = pred_head or primary or (next(iter(heads)) if len(heads) == 1 else None)
            if head is not None:
                target_slice = resolve_head_target_slice(cfg, head)
        # the reference's spellings (training/losses/plan.py:126-147): coefficient = weight, pred / target / mask = *_slice
        plan.append({"fn": fn, "row": row, "loss": loss, "weight": float(get("coefficient", get("weight", 1.0))),
                     "pred_head": pred_head, "pred_slice": pred_slice, "call_kind": call_kind, "pred2_slice": pred2_slice,
                     "pred2_head": pred2_head, "spatial_arg": row.spatial, "target_slice": target_slice, "pos_weight": pos_weight,
                     "target_kind": row.target, "mask_slice": get("mask_slice", get("mask")),
                     "apply_deep_supervision": bool(get("apply_deep_supervision", True)), "kwargs": kwargs})
    return plan


class ConnectomicsModule(nn.Module):
    def __init__(self, cfg, model: Optional[nn.Module] = None):
        super().__init__()
        self.cfg = cfg
        self.model = model if model is not None else build_model(cfg)
        loss_cfg = getattr(cfg.model, "loss", None)
        self.deep_supervision = bool(getattr(loss_cfg, "deep_supervision", False))
        self.ds_weights = list(getattr(loss_cfg, "deep_supervision_weights", None) or DS_WEIGHTS)
        self.loss_terms = plan_loss_terms(cfg)
        # adaptive loss balancing (reference training/losses/balancing.py:64-222; tutorials/mitoEM/common.yaml:54-55): a trainable
        # sub-module, every loss entry is one task.  `uncertainty` rides on the fused loss kernel (the learned task coefficients
        # enter it as host scalars, _balanced_scale_loss); `gradnorm` needs every task's own graph and takes the generic path
        from .balancing import build_loss_weighter
        self.loss_weighter = build_loss_weighter(cfg, len(self.loss_terms), self.model)
        self.fused_loss = bool(getattr(loss_cfg, "fused", True))
        # every prediction is clamped before its loss, at every scale (orchestrator.py:95-96,574; schema/model.py:50-51)
        self.clamp_min = float(getattr(loss_cfg, "deep_supervision_clamp_min", -20.0))
        self.clamp_max = float(getattr(loss_cfg, "deep_supervision_clamp_max", 20.0))
        self.global_step = 0
        self.current_epoch = 0
        self._val_state: Optional[ConfusionState] = None     # the validation epoch's table of counts (evaluation.enabled with metrics)
        self.val_history: list = []                          # what fit() appends after every validate()

    # ---- reference-visible methods ----------------------------------------------------------------
    def forward(self, x: torch.Tensor):
        return self.model(x)

    def _term_is_fusable(self, t, pred) -> bool:
        """The fused kernel computes mean-reduced BCE-with-logits (numeric pos_weight) and sigmoid Dice with MONAI's default
        smoothing over all channels; any other variant of those terms takes the generic path."""
        kind = t["row"].fused
        if kind is None or t.get("mask_slice") is not None:
            return False
        kw = t["kwargs"]
        if kind == "bce":
            return not isinstance(t["pos_weight"], str) and str(kw.get("reduction", "mean")) == "mean" and \
                not (set(kw) - {"reduction"})
        smooth_ok = abs(float(kw.get("smooth_nr", 1e-5)) - 1e-5) < 1e-12 and abs(float(kw.get("smooth_dr", 1e-5)) - 1e-5) < 1e-12
        bg_ok = bool(kw.get("include_background", True)) or pred.shape[1] == 1
        return bool(kw.get("sigmoid", False)) and smooth_ok and bg_ok and not kw.get("squared_pred", False) and \
            not (set(kw) - {"sigmoid", "smooth_nr", "smooth_dr", "include_background", "squared_pred"})

    def _term_label_mask(self, t, label_mask):
        """The channels of the label mask a term's targets come from: its `target_slice`, or all of them."""
        if t["target_slice"] is None:
            return label_mask
        return label_mask[:, resolve_channel_indices(t["target_slice"], num_channels=label_mask.shape[1], context="target_slice")]

    def _fused_term_loss(self, pred, target, mask, terms, label_mask=None):
        """All terms are BCE-with-logits / sigmoid-Dice: one fused HIP reduction per (pred_slice, target_slice) pair."""
        from .fused import bce_dice_loss
        groups = {}
        for i, t in terms:
            key = (str(t["pred_slice"]), str(t["target_slice"]))
            g = groups.setdefault(key, {"bce": None, "dice": None, "t": t})
            kind = t["row"].fused
            if g[kind] is not None:
                return None                   # two terms of one kind on the same slices: take the generic path
            g[kind] = (i, t)
        total, parts = 0.0, {}
        for g in groups.values():
            t = g["t"]
            p, y = pred, target
            if t["pred_slice"] is not None:
                p = pred[:, resolve_channel_indices(t["pred_slice"], num_channels=pred.shape[1], context="pred_slice")]
            if t["target_slice"] is not None:
                y = target[:, resolve_channel_indices(t["target_slice"], num_channels=target.shape[1], context="target_slice")]
            wb = g["bce"][1]["weight"] if g["bce"] else 0.0
            wd = g["dice"][1]["weight"] if g["dice"] else 0.0
            pw = g["bce"][1]["pos_weight"] if g["bce"] else None        # (None for a loss without a weight map: plan_loss_terms)
            m = mask
            if label_mask is not None:
                # the term's channels of the label mask join the batch mask; the kernel reads the product as its per-channel weight
                lm = self._term_label_mask(t, label_mask)
                y = torch.where(lm > 0, y, torch.zeros_like(y))
                m = lm if mask is None else mask * lm
            v, out = bce_dice_loss(p, y, m, w_bce=wb, w_dice=wd, pos_weight=pw)
            if g["bce"]:
                parts[f"loss_{g['bce'][0]}_{g['bce'][1]['fn']}"] = out[1]
            if g["dice"]:
                parts[f"loss_{g['dice'][0]}_{g['dice'][1]['fn']}"] = out[2]
            total = total + v
        return total, parts

    def _fusable(self, pred, mask, terms) -> bool:
        # (a BCE that sees a mask through its inputs -- torch's BCEWithLogitsLoss -- averages over ALL voxels, masked ones as logit -20 /
        # target 0, which the fused kernel's valid-voxel mean is not)
        plain_bce_masked = mask is not None and any(t["row"].fused == "bce" and t["row"].spatial is None for _, t in terms)
        return bool(pred.is_cuda and self.fused_loss and not plain_bce_masked and all(self._term_is_fusable(t, pred) for _, t in terms))

    def _term_loss(self, pred, target, mask=None, terms=None, tasks=None, heads=None, full_labels=None, label_mask=None):
        """Weighted sum of the loss terms `terms` (list of (index, term); default: all) on one prediction tensor.
        tasks: a dict that receives {term index: static weight x raw value, WITH its graph} (adaptive balancing: the caller
        combines the tasks); the fused kernel steps aside then -- it returns one scalar for all its terms.
        heads: the named-head outputs, for a `pred_pred` term whose second slice comes from another head.
        full_labels: on a deep-supervision scale, the labels at full resolution: a `class_index` term (CrossEntropyLoss) resizes ITS
        channel of them by nearest neighbour (orchestrator.py:277-291, 578-586) instead of reading the densely resized `target`.
        label_mask: the label transform's per-channel valid mask (float 0 / 1, at this scale): every supervised term multiplies its
        `target_slice` channels of it into its valid mask; None takes the path without one, unchanged."""
        terms = list(enumerate(self.loss_terms)) if terms is None else terms
        pred = torch.clamp(pred, min=self.clamp_min, max=self.clamp_max)
        total, parts = 0.0, {}
        if tasks is None:
            # the terms without a target (regularisers) never enter the fused reduction and must not push the supervised terms off
            # it: those are judged on their own, the rest is added below
            # (nor do the softmax losses and L1Loss, which have kernels or rows of their own)
            supervised = [(i, t) for i, t in terms if not t["row"].beside_fused]
            if supervised and self._fusable(pred, mask if mask is not None else label_mask, supervised):
                res = self._fused_term_loss(pred, target, mask, supervised, label_mask)   # finiteness is checked where fit() reads the value
                if res is not None:
                    if len(supervised) == len(terms):
                        return res
                    total, parts = res
                    terms = [(i, t) for i, t in terms if t["row"].beside_fused]
        for i, t in terms:
            v = self._supervised_loss(i, t, pred, target, mask, full_labels, label_mask) if t["row"].call == "pred_target" else \
                self._regularizer_loss(i, t, pred, target, mask, heads)
            if not torch.isfinite(v):
                raise FloatingPointError(f"loss term {t['fn']} is not finite")
            parts[f"loss_{i}_{t['fn']}"] = v.detach()
            if tasks is not None:
                tasks[i] = t["weight"] * v
            total = total + t["weight"] * v
        return total, parts

    def _supervised_loss(self, i, t, pred, target, mask, full_labels, label_mask=None):
        """A `pred_target` term on the clamped predictions: its slices, its target form and its spatial argument."""
        row = t["row"]
        p, y = pred, target
        if t["pred_slice"] is not None:
            p = pred[:, resolve_channel_indices(t["pred_slice"], num_channels=pred.shape[1], context="pred_slice")]
        if row.target == "class_index" and full_labels is not None:
            y = full_labels
        if t["target_slice"] is not None:
            y = y[:, resolve_channel_indices(t["target_slice"], num_channels=y.shape[1], context="target_slice")]
        if row.target == "class_index":
            if y.dim() != pred.dim() or y.shape[1] != 1:
                raise ValueError(f"Loss term 'loss_{i}_{t['fn']}' takes a class-index target of one channel, got "
                                 f"{tuple(y.shape)} (name it with target_slice)")
            y = resize_class_index_to_output(y, pred)
        if label_mask is not None:
            # the transform's valid mask of the term's target channels (orchestrator.py:492-498, 635-648): a factor of everything
            # the batch mask is a factor of, and invalid targets read as 0
            lm = self._term_label_mask(t, label_mask)
            y = torch.where(lm > 0, y, torch.zeros_like(y))
            mask = lm if mask is None else mask * lm
        # what the loss sees as its spatial argument (reference orchestrator.py:566-646): a term's own mask channels
        # (`mask_slice` of the labels) x the batch mask; a `weight`-taking loss without a mask of its own gets the
        # class-balancing map instead (unless its pos_weight is a scalar of its own)
        own = None
        if t.get("mask_slice") is not None:
            own = target[:, resolve_channel_indices(t["mask_slice"], num_channels=target.shape[1], context="mask_slice")]
        valid = own if mask is None else (mask if own is None else own * mask)
        if row.spatial != "weight":
            return t["loss"](p, y, valid, fill=self.clamp_min)
        spatial, pw = own, None
        if spatial is None and row.balance_map:
            spatial = class_balance_weight(y, 1.0 if (t["pos_weight"] is None and row.own_pos_weight) else t["pos_weight"],
                                           valid_mask=valid)
        if mask is not None:
            spatial = mask if spatial is None else spatial * mask
        if not row.balance_map:
            pw = t["pos_weight"]
            if isinstance(pw, str):
                pw = auto_pos_weight_scalar(y, valid)
            elif pw is not None and float(pw) == 1.0:
                pw = None
        return t["loss"](p, y, spatial, fill=self.clamp_min, pos_weight=pw)

    def _regularizer_loss(self, i, t, pred, target, mask, heads):
        """A `pred_only` / `pred_pred` term (training/losses/orchestrator.py:533-718): one or two slices of the clamped predictions
        -- the second from `pred2_head` when the model has named heads --, no target, and as `mask` the term's `mask_slice` channels
        of the labels x the batch mask, for the losses that take one."""
        args = [pred[:, resolve_channel_indices(t["pred_slice"], num_channels=pred.shape[1], context="pred_slice")]]
        if t["call_kind"] == "pred_pred":
            src = pred
            if heads is not None and t.get("pred2_head") is not None:
                if t["pred2_head"] not in heads:
                    raise ValueError(f"Loss term 'loss_{i}_{t['fn']}' requested pred2_head='{t['pred2_head']}', but available output "
                                     f"heads are {sorted(heads)}.")
                src = torch.clamp(heads[t["pred2_head"]], min=self.clamp_min, max=self.clamp_max)
            args.append(src[:, resolve_channel_indices(t["pred2_slice"], num_channels=src.shape[1], context="pred2_slice")])
        combined = None
        if t.get("mask_slice") is not None:
            combined = target[:, resolve_channel_indices(t["mask_slice"], num_channels=target.shape[1], context="mask_slice")]
        if mask is not None:
            combined = mask if combined is None else combined * mask
        if t["spatial_arg"] == "mask" and combined is not None:
            v = t["loss"](*args, mask=combined)
        else:
            v = t["loss"](*args)
        return v

    def _balanced_scale_loss(self, items, stage: str, heads=None, full_labels=None, label_mask=None):
        """One output scale under adaptive loss balancing (orchestrator.py:110-127, 779-790): `items` = [(pred, target, mask, terms)]
        (one entry per head); every term is a task whose loss is its static weight x raw value, the weighter combines ALL tasks of
        the scale in one call.  Uncertainty weighting on fusable terms keeps the fused HIP loss: the per-task coefficients
        0.5 * exp(-s_i) multiply the static weights as host scalars (one device -> host read of T floats per scale), the kernel's
        scalar is sum_i coef_i * task_i exactly, and the gradient of the log-variances -- which the kernel knows nothing of -- comes
        from a zero-valued term built on the detached task values."""
        from .balancing import UncertaintyLossWeighter
        w = self.loss_weighter
        idx = sorted(i for _, _, _, terms in items for i, _ in terms)
        if idx != list(range(len(self.loss_terms))):
            raise ValueError(f"adaptive loss balancing combines all {len(self.loss_terms)} loss terms at every scale it sees; this scale "
                             f"carries terms {idx} (apply_deep_supervision: false on a term is not compatible with loss_balancing)")
        names = [f"loss_{i}_{self.loss_terms[i]['fn']}" for i in idx]
        parts: Dict[str, Any] = {}
        if isinstance(w, UncertaintyLossWeighter) and all(self._fusable(torch.clamp(p, self.clamp_min, self.clamp_max),
                                                                        m if m is not None else label_mask, terms)
                                                           for p, _, m, terms in items):
            coef = 0.5 * torch.exp(-w.log_vars)
            host = [float(c) for c in coef.detach().cpu().tolist()]
            fused_total, ok = 0.0, True
            raw: Dict[int, torch.Tensor] = {}
            for pred, target, mask, terms in items:
                scaled = [(i, {**t, "weight": t["weight"] * host[i]}) for i, t in terms]
                res = self._fused_term_loss(torch.clamp(pred, min=self.clamp_min, max=self.clamp_max), target, mask, scaled, label_mask)
                if res is None:
                    ok = False
                    break
                fused_total = fused_total + res[0]
                for i, t in terms:
                    raw[i] = res[1][f"loss_{i}_{t['fn']}"]
                parts.update(res[1])
            if ok:
                tasks = torch.stack([self.loss_terms[i]["weight"] * raw[i].detach().float().reshape(()) for i in idx])
                total = fused_total + ((coef - coef.detach()) * tasks).sum() + 0.5 * w.log_vars.sum()
                wts = torch.exp(-w.log_vars).detach()
                for n, wt in zip(names, wts):
                    parts[f"{n}_balance_weight"] = wt
                    parts[f"{stage}_loss_uncertainty/{n}_weight"] = wt
                parts[f"{stage}_loss_uncertainty/reg"] = (0.5 * w.log_vars.sum()).detach()
                return total, parts
            parts = {}
        tasks: Dict[int, torch.Tensor] = {}
        for pred, target, mask, terms in items:
            _, pr = self._term_loss(pred, target, mask, terms, tasks=tasks, heads=heads, full_labels=full_labels, label_mask=label_mask)
            parts.update(pr)
        total, wts, logs = w.combine([tasks[i] for i in idx], names, stage)
        for n, wt in zip(names, wts):
            parts[f"{n}_balance_weight"] = wt
        parts.update(logs)
        return total, parts

    def _head_of(self, term_index: int, term, heads) -> str:
        """Which named head a term reads (training/losses/orchestrator.py:328-378): its pred_head, else
        model.primary_head, else the only head; anything else is a configuration error."""
        want = term["pred_head"]
        if want is None:
            primary = getattr(self.cfg.model, "primary_head", None)
            if primary is not None and primary in heads:
                want = primary
            elif len(heads) == 1:
                want = next(iter(heads))
            else:
                raise ValueError(f"Loss term 'loss_{term_index}_{term['fn']}' did not specify pred_head and model.primary_head "
                                 f"is unset, but model output has multiple heads {sorted(heads)}.")
        if want not in heads:
            raise ValueError(f"Loss term 'loss_{term_index}_{term['fn']}' requested pred_head='{want}', but available output "
                             f"heads are {sorted(heads)}.")
        if not isinstance(heads[want], torch.Tensor):
            raise TypeError(f"Output head '{want}' must be a tensor, got {type(heads[want]).__name__}.")
        return want

    def _compute_loss(self, outputs, labels, mask=None, label_mask=None):
        stage = "train" if self.training else "val"
        if label_mask is not None:
            label_mask = check_label_mask(label_mask, labels)
        main = unwrap_main_output(outputs)
        if isinstance(main, dict):
            # named heads: every term reads its own head; the terms of one head share a (fused) reduction
            if not main:
                raise ValueError("Named-head model output mapping is empty.")
            by_head: Dict[str, list] = {}
            for i, t in enumerate(self.loss_terms):
                by_head.setdefault(self._head_of(i, t, main), []).append((i, t))
            total, parts = 0.0, {}
            if self.loss_weighter is not None:
                total, parts = self._balanced_scale_loss([(main[head], labels, mask, terms) for head, terms in by_head.items()], stage,
                                                         heads=main, label_mask=label_mask)
            else:
                for head, terms in by_head.items():
                    v, pr = self._term_loss(main[head], labels, mask, terms, heads=main, label_mask=label_mask)
                    total = total + v
                    parts.update(pr)
            total = self.ds_weights[0] * total
            parts["train_loss_total"] = total.detach()
            return total, parts
        for i, t in enumerate(self.loss_terms):
            if t["pred_head"] is not None:
                raise ValueError(f"Loss term 'loss_{i}_{t['fn']}' requested pred_head='{t['pred_head']}' but the model "
                                 "output is a single tensor.")
            if t.get("pred2_head") is not None:
                raise ValueError(f"Loss term 'loss_{i}_{t['fn']}' requested pred2_head='{t['pred2_head']}' but the model "
                                 "output is a single tensor.")
        all_terms = list(enumerate(self.loss_terms))
        if self.loss_weighter is not None:
            total, parts = self._balanced_scale_loss([(main, labels, mask, all_terms)], stage, label_mask=label_mask)
        else:
            total, parts = self._term_loss(main, labels, mask, label_mask=label_mask)
        total = self.ds_weights[0] * total
        if self.deep_supervision and isinstance(outputs, dict):
            for i in range(1, 5):
                ds = outputs.get(f"ds_{i}")
                if ds is None:
                    continue
                tgt = match_target_to_output(labels, ds)
                m = None if mask is None else resize_class_index_to_output(mask, ds)
                lm = None if label_mask is None else resize_label_mask_to_output(label_mask, ds)
                on_scales = [(j, t) for j, t in enumerate(self.loss_terms) if t.get("apply_deep_supervision", True)]
                if not on_scales:
                    continue
                if self.loss_weighter is not None:
                    li, _ = self._balanced_scale_loss([(ds, tgt, m, on_scales)], stage, full_labels=labels, label_mask=lm)
                else:
                    li, _ = self._term_loss(ds, tgt, m, on_scales, full_labels=labels, label_mask=lm)
                total = total + self.ds_weights[i] * li
        parts["train_loss_total"] = total.detach()
        return total, parts

    def training_step(self, batch: Dict[str, torch.Tensor], batch_idx: int = 0) -> torch.Tensor:
        outputs = self(batch["image"])
        loss, self.last_log = self._compute_loss(outputs, batch["label"], batch.get("mask"), batch.get("label_mask"))
        return loss

    # ---- the `evaluation` block: voxel metrics of a validation epoch (training/metrics.py) ------------
    def _evaluation_request(self):
        """-> (the metric names `evaluation` asks for, or None when it is disabled or lists none; prediction_threshold)."""
        ev = getattr(self.cfg, "evaluation", None)
        names = _cfg_get(ev, "metrics", None)
        if ev is None or not bool(_cfg_get(ev, "enabled", False)) or not names:
            return None, 0.5
        return [str(n) for n in names], float(_cfg_get(ev, "prediction_threshold", 0.5))

    def _has_multiple_supervised_loss_tasks(self) -> bool:
        return sum(1 for t in self.loss_terms if t["call_kind"] == "pred_target") > 1

    def _validation_state(self) -> ConfusionState:
        """The epoch's table, sized as the reference sizes its validation metrics (lightning/model.py:551-563): the selected named
        head's width; else binary for a multi-task loss or one output channel, `model.out_channels` classes otherwise."""
        if self._val_state is None:
            heads = getattr(self.cfg.model, "heads", None) or {}
            named = None
            if heads:
                head = resolve_configured_output_head(self.cfg, purpose="validation metric setup", allow_none=True)
                if head is not None and head in heads:
                    named = int(_cfg_get(heads[head], "out_channels", 0))
            if named is not None:
                num_classes, use_binary = named, named == 1
            else:
                num_classes = int(getattr(self.cfg.model, "out_channels", 2))
                use_binary = self._has_multiple_supervised_loss_tasks() or num_classes == 1
            self._val_state = ConfusionState(1 if use_binary else num_classes)
        return self._val_state

    def _resolve_validation_target_slice(self, head_name: str):
        """The label slice a named head is supervised with (lightning/model.py:372-400): the head's own `target_slice`, else the one
        target slice its pred_target loss terms agree on."""
        explicit = resolve_head_target_slice(self.cfg, head_name)
        if explicit is not None:
            return explicit
        primary = getattr(self.cfg.model, "primary_head", None)
        matching = []
        for t in self.loss_terms:
            if t["call_kind"] != "pred_target":
                continue
            if (t["pred_head"] if t["pred_head"] is not None else primary) == head_name and t["target_slice"] not in matching:
                matching.append(t["target_slice"])
        if not matching:
            raise ValueError(f"Validation metric computation could not find any pred_target loss term for head '{head_name}'.")
        if len(matching) > 1:
            raise ValueError(f"Validation metric computation found multiple target slices for head '{head_name}': {matching}. "
                             "Configure a single supervised label slice for the evaluated head.")
        return matching[0]

    @staticmethod
    def _prepare_metric_predictions(prediction: torch.Tensor, target: torch.Tensor):
        """-> (prediction, target, target_mode) as the count kernel reads them (lightning/model.py:403-432): one output channel is
        thresholded against a one-channel class label; several are an argmax against a class-index channel or as many one-hot channels."""
        if int(prediction.shape[1]) == 1:
            if int(target.shape[1]) != 1:
                raise ValueError(f"Binary metric computation expects a single target channel, got {tuple(target.shape)}.")
            return prediction, target, "index"
        if int(target.shape[1]) == 1:
            return prediction, target, "index"
        if int(target.shape[1]) == int(prediction.shape[1]):
            return prediction, target, "dense"
        raise ValueError("Multiclass metric computation requires either a single class-index target channel or the same number of "
                         f"one-hot channels as the prediction. Got prediction.shape={tuple(prediction.shape)} and "
                         f"target.shape={tuple(target.shape)}.")

    def _select_metric_operands(self, outputs, labels: torch.Tensor):
        """The reference's choice of what a validation metric compares (lightning/model.py:935-981), as views: nothing is copied."""
        purpose = "validation metric computation"
        requested = resolve_configured_output_head(self.cfg, purpose=purpose, allow_none=True)
        main, head = select_output_tensor(outputs, requested_head=requested, primary_head=getattr(self.cfg.model, "primary_head", None),
                                          purpose=purpose)
        if head is not None:
            target_slice = self._resolve_validation_target_slice(head)
            target = labels
            if target_slice is not None:
                a, b = resolve_channel_range(target_slice, num_channels=int(labels.shape[1]),
                                             context=f"validation target slice for head '{head}'")
                target = labels[:, a:b]
            return self._prepare_metric_predictions(main, target)
        if self._has_multiple_supervised_loss_tasks():
            return main[:, 0:1], labels[:, 0:1], "index"          # a multi-task output: channel 0 of both, as a binary metric
        if int(labels.shape[1]) != 1:
            raise ValueError(f"Validation metric computation expects a single class-label channel, got {tuple(labels.shape)}.")
        return main, labels, "index"

    @torch.no_grad()
    def validation_step(self, batch, batch_idx: int = 0) -> Dict[str, torch.Tensor]:
        outputs = self(batch["image"])
        loss, _ = self._compute_loss(outputs, batch["label"], batch.get("mask"), batch.get("label_mask"))
        names, threshold = self._evaluation_request()
        if names is None:
            main = unwrap_main_output(outputs)
            p = torch.sigmoid(main[:, :1].float()) > 0.5
            t = batch["label"][:, :1] > 0
            union = (p | t).sum().clamp_min(1)
            return {"val_loss_total": loss, "val_jaccard": (p & t).sum().float() / union}
        # the RAW output against prediction_threshold, no sigmoid: what the reference does (lightning/model.py:416, 974-981)
        pred, target, mode = self._select_metric_operands(outputs, batch["label"])
        self._validation_state().update(pred, target, pred_threshold=threshold, target_mode=mode)
        return {"val_loss_total": loss}

    def validation_epoch_end(self, _riders: Optional[torch.Tensor] = None):
        """The epoch's `val_<name>` values from the table of counts (summed over the ranks), which is then reset.  `_riders`
        (validate()): device scalars read in the same host copy; they come back as floats, second in a tuple."""
        names, _ = self._evaluation_request()
        state = self._val_state
        if names is None or state is None or state.counts is None:
            return {} if _riders is None else ({}, [float(v) for v in _riders.reshape(-1).tolist()])
        state.all_reduce()
        if _riders is None:
            out = {f"val_{k}": v for k, v in state.compute(names).items()}
            state.reset()
            return out
        # counts stay exact in float64 below 2^53 voxels
        packed = torch.cat([state.counts.to(torch.float64), _riders.detach().reshape(-1).to(state.counts.device, torch.float64)]).cpu()
        n = state.counts.numel()
        out = {f"val_{k}": v for k, v in metrics_from_counts(packed[:n].to(torch.int64), state.num_classes, names).items()}
        state.reset()
        return out, [float(v) for v in packed[n:].tolist()]

    def configure_optimizers(self):
        # with an adaptive loss weighter the optimizer takes the whole module (its task weights train with the network), as the
        # reference does (lightning/model.py:1160-1162)
        opt = build_optimizer(self.cfg, self if self.loss_weighter is not None else self.model)
        return opt, build_lr_scheduler(self.cfg, opt)

    # ---- checkpoints in the Lightning layout ------------------------------------------------------
    def checkpoint_dict(self, optimizer=None) -> Dict[str, Any]:
        sd = {"model." + k: v.detach().cpu() for k, v in self.model.state_dict().items()}
        if self.loss_weighter is not None:      # a sub-module of the LightningModule in the reference: same key prefix
            sd.update({"loss_weighter." + k: v.detach().cpu() for k, v in self.loss_weighter.state_dict().items() if v is not None})
            if getattr(self.loss_weighter, "initial_losses", None) is not None:
                sd["loss_weighter.initial_losses"] = self.loss_weighter.initial_losses.detach().cpu()
        ck = {"state_dict": sd,
              "global_step": self.global_step,
              "pytc_metadata": {"format_version": 1, "model_arch": str(getattr(self.cfg.model.arch, "type", ""))}}
        ck["epoch"] = int(getattr(self, "current_epoch", 0))
        sched = getattr(self, "_scheduler", None)
        if sched is not None:
            ck["lr_schedulers"] = [sched.state_dict()]
        if optimizer is not None:
            ck["optimizer_states"] = [optimizer.state_dict()]
            if getattr(optimizer, "ema", None):
                # the reference persists the EMA under its callback's state (callbacks.py:732-790: "ema_state",
                # "updates", "decay"); same vocabulary here so either side can resume / evaluate with it
                ck["callbacks"] = {"EMAWeightsCallback": {
                    "ema_state": {k: v.cpu() for k, v in optimizer.ema_state_dict(self.model).items()},
                    "updates": int(optimizer.ema_updates), "decay": float(optimizer.ema_decay)}}
        return ck

    def load_checkpoint_dict(self, ck: Dict[str, Any]) -> None:
        """Model weights + counters now; optimizer / scheduler / EMA state is kept and applied by `restore_training_state`
        once `fit` has built them (a true resume: Adam moments, the LR schedule position and the EMA shadow continue)."""
        sd = {k[len("model."):]: v for k, v in ck["state_dict"].items()
              if k.startswith("model.") and not k.startswith("model.loss_functions.")}
        wsd = {k[len("loss_weighter."):]: v for k, v in ck["state_dict"].items() if k.startswith("loss_weighter.")}
        if wsd and self.loss_weighter is None:
            import warnings
            warnings.warn(f"checkpoint carries adaptive loss-balancing state ({len(wsd)} tensors, e.g. 'loss_weighter.{sorted(wsd)[0]}') but "
                          "model.loss.loss_balancing is not configured: the learned task weights are NOT restored", RuntimeWarning, stacklevel=2)
        elif wsd:
            if "initial_losses" in wsd and hasattr(self.loss_weighter, "initial_losses"):
                # (a None buffer cannot be load_state_dict'ed; a checkpointed reference point always replaces the live one)
                self.loss_weighter.initial_losses = wsd["initial_losses"].clone()
            bad = self.loss_weighter.load_state_dict({k: v for k, v in wsd.items() if k != "initial_losses"}, strict=False)
            missing_w = [k for k in bad.missing_keys if k != "initial_losses"]
            if bad.unexpected_keys or missing_w:
                raise RuntimeError(f"checkpoint loss_weighter state does not match the configured strategy: unexpected "
                                   f"{bad.unexpected_keys}, missing {missing_w}")
        missing, unexpected = self.model.load_state_dict(sd, strict=False)
        # a reference checkpoint may carry deep-supervision heads of a trunk built with them (`out_1..out_4`); anything else
        # missing / unexpected is an architecture mismatch
        bad_unexpected = [k for k in unexpected if not any(f".out_{i}." in "." + k for i in (1, 2, 3, 4))]
        if missing or bad_unexpected:
            raise RuntimeError(f"checkpoint does not match the model: missing {missing[:5]}, unexpected {bad_unexpected[:5]}")
        self.global_step = int(ck.get("global_step", 0))
        self.current_epoch = int(ck.get("epoch", 0))
        self._resume = {k: ck[k] for k in ("optimizer_states", "lr_schedulers", "callbacks") if k in ck}

    def restore_training_state(self, optimizer, scheduler=None) -> bool:
        """Apply the optimizer / scheduler / EMA state of a loaded checkpoint.  Optimizer states written with the reference's
        one-group-per-parameter layout (or torch's) are remapped by parameter order onto this optimizer's merged groups."""
        res = getattr(self, "_resume", None)
        if not res:
            return False
        if res.get("optimizer_states"):
            _load_optimizer_state(optimizer, res["optimizer_states"][0])
        if scheduler is not None and res.get("lr_schedulers"):
            scheduler.load_state_dict(res["lr_schedulers"][0])
        ema = _ema_callback_entry(res)
        if ema and getattr(optimizer, "ema_decay", None) is not None and hasattr(optimizer, "load_ema_state_dict"):
            optimizer.load_ema_state_dict(self.model, ema[EMA_STATE_KEY], int(ema.get("updates", 0)))
        self._resume = None
        return True


EMA_STATE_KEY = "ema_state"                    # the reference callback's vocabulary (callbacks.py:752 `EMAWeightsCallback.EMA_STATE_KEY`)


def _ema_callback_entry(checkpoint: Dict[str, Any]) -> Optional[Dict[str, Any]]:
    """The EMA callback's state inside a Lightning-layout checkpoint: Lightning keys callback states by `state_key`, the class name
    optionally followed by its arguments, hence the prefix match (reference callbacks.py:54-59)."""
    for key, state in (checkpoint.get("callbacks") or {}).items():
        if isinstance(state, dict) and str(key).startswith("EMAWeightsCallback") and state.get(EMA_STATE_KEY):
            return state
    return None


def load_ema_state_dict(checkpoint: Dict[str, Any]) -> Optional[Dict[str, torch.Tensor]]:
    """The EMA weights stored in `checkpoint`, keyed like `model.state_dict()`; None when the run had EMA off or the checkpoint
    carries none (reference training/lightning/callbacks.py:46-60 -- same contract, so `--ema` evaluation reads either side's files)."""
    entry = _ema_callback_entry(checkpoint)
    return dict(entry[EMA_STATE_KEY]) if entry else None


def _load_optimizer_state(optimizer, state: Dict[str, Any]) -> None:
    """optimizer.load_state_dict that tolerates a different GROUPING of the same parameters in the same order: torch maps
    saved state to parameters by position, so the per-parameter state (exp_avg, exp_avg_sq, step) is re-keyed onto this
    optimizer's parameter order and the groups keep their own hyper-parameters (the checkpoint's lr is adopted per
    parameter when the group counts match, as torch would)."""
    saved_groups = state["param_groups"]
    own_groups = optimizer.state_dict()["param_groups"]
    n_saved = sum(len(g["params"]) for g in saved_groups)
    n_own = sum(len(g["params"]) for g in own_groups)
    if n_saved != n_own:
        raise ValueError(f"optimizer state holds {n_saved} parameters, the optimizer {n_own}: different models")
    if [len(g["params"]) for g in saved_groups] == [len(g["params"]) for g in own_groups]:
        optimizer.load_state_dict(state)
        return
    # position of every parameter in the model-order enumeration both layouts were built from
    order_own = [pid for g in own_groups for pid in g["params"]]
    if len(saved_groups) == n_saved:                 # reference layout: one group per parameter, in model order
        order_saved = [g["params"][0] for g in saved_groups]
        model_pos_of_own = _model_order_positions(optimizer)
        remap = {order_saved[model_pos_of_own[i]]: order_own[i] for i in range(n_own)}
    else:
        raise ValueError("optimizer state has a parameter grouping this loader cannot remap "
                         f"({len(saved_groups)} groups for {n_saved} parameters)")
    new_state = {remap[k]: v for k, v in state["state"].items() if k in remap}
    optimizer.load_state_dict({"state": new_state, "param_groups": own_groups})


def _model_order_positions(optimizer):
    """For the i-th parameter in the optimizer's flattened group order: its index in model (registration) order."""
    order = getattr(optimizer, "_pytc_model_order", None)
    if order is None:
        raise ValueError("the optimizer does not know the model order of its parameters (built outside build_optimizer)")
    flat = [p for g in optimizer.param_groups for p in g["params"]]
    return [order[id(p)] for p in flat]


def precision_to_dtype(precision) -> torch.dtype:
    """Lightning precision strings: 16-mixed / bf16-mixed -> bf16 storage on this engine; 32 -> fp32."""
    return torch.bfloat16 if any(s in str(precision) for s in ("16", "bf16")) else torch.float32


def resolve_training_steps(cfg, *, fast_dev_run: int = 0, dataset_steps_per_epoch: Optional[int] = None) -> tuple[int, int]:
    """(total optimizer steps, steps per epoch) from optimization.{max_steps, max_epochs, n_steps_per_epoch}.  The reference's
    default n_steps_per_epoch = -1 means "from the dataset size" (schema/optimization.py:96): with an iterable synthetic /
    sampled source there is no such size, so `dataset_steps_per_epoch` (when the caller knows one) or an explicit error."""
    oc = cfg.optimization
    if fast_dev_run:
        return int(fast_dev_run), int(fast_dev_run)
    per_epoch = getattr(oc, "n_steps_per_epoch", None)
    per_epoch = int(per_epoch) if per_epoch is not None else -1
    max_steps = getattr(oc, "max_steps", None)
    if per_epoch <= 0 and (dataset_steps_per_epoch is None or dataset_steps_per_epoch <= 0) \
            and max_steps is not None and int(max_steps) > 0:
        # no epoch length from either side, but a total: the run is one "epoch" of max_steps optimizer steps
        return int(max_steps), int(max_steps)
    if per_epoch <= 0:
        if dataset_steps_per_epoch is None or dataset_steps_per_epoch <= 0:
            raise ValueError("optimization.n_steps_per_epoch is -1 / unset (auto from the dataset size) but the training source "
                             "is an endless sampler: set optimization.n_steps_per_epoch (or optimization.max_steps)")
        per_epoch = int(dataset_steps_per_epoch)
    total = per_epoch * max(1, int(getattr(oc, "max_epochs", 1) or 1))
    if max_steps is not None and int(max_steps) > 0:
        total = min(total, int(max_steps)) if getattr(oc, "max_epochs", None) else int(max_steps)
    return total, per_epoch


def validate(module: ConnectomicsModule, batches, *, device, max_batches: Optional[int] = None) -> Dict[str, float]:
    """One validation epoch over `batches` (at most `max_batches` of them) in eval mode under no_grad; the module's previous mode is
    restored.  -> the mean of every value `validation_step` returns (`val_loss_total`; `val_jaccard` with evaluation off) plus the
    epoch metrics of `validation_epoch_end` (`val_jaccard` / `val_dice` / `val_accuracy` with evaluation on).  Nothing is read back
    per batch: the sums and the table of counts reach the host in one copy at the end."""
    was_training = module.training
    module.eval()
    sums: Dict[str, torch.Tensor] = {}
    n = 0
    try:
        with torch.no_grad():
            for i, batch in enumerate(batches):
                if max_batches is not None and i >= int(max_batches):
                    break
                batch = {k: v.to(device, non_blocking=True) for k, v in batch.items()}
                for k, v in module.validation_step(batch, i).items():
                    v = v.detach().to(torch.float64)
                    sums[k] = v if k not in sums else sums[k] + v
                n += 1
            if n == 0:
                raise ValueError("validate: no validation batches")
            keys = sorted(sums)
            metrics, host = module.validation_epoch_end(torch.stack([sums[k].reshape(()) for k in keys]))
    finally:
        module.train(was_training)
    out = {k: v / n for k, v in zip(keys, host)}
    out.update(metrics)
    return out


def fit(module: ConnectomicsModule, batches, *, max_steps: int, device, log_every: int = 10, ddp: bool = False,
        log=print, steps_per_epoch: Optional[int] = None, val_batches=None, val_every: Optional[int] = None):
    """Minimal training loop: forward (HIP) -> loss -> backward (HIP) -> clip -> optimizer (+ scheduler).
    With `val_batches` (a re-iterable collection of batches) and `val_every`, `validate` runs every `val_every` optimizer steps and
    after the last one; each result is logged and appended, with its step, to `module.val_history`.
    `batches` yields {"image","label"[,"mask"][,"label_mask"]} dicts of (B,C,D,H,W) tensors.  `max_steps` is the TOTAL step count of the run:
    after `load_checkpoint_dict` the loop continues from `module.global_step` with the optimizer moments, the scheduler
    position and the EMA shadow of the checkpoint.  The scheduler steps per `optimization.scheduler.interval` ('epoch', the
    reference default, every `steps_per_epoch` optimizer steps; or 'step') and `frequency` (lightning/model.py:1174-1200)."""
    cfg = module.cfg
    module.to(device).train()
    inner = getattr(module.model, "model", module.model)
    dt = precision_to_dtype(getattr(cfg.optimization, "precision", "32"))
    for mod in (module.model, inner):
        if hasattr(mod, "compute_dtype"):
            mod.compute_dtype = dt
    net = module
    weighter_params = []
    if ddp:
        from torch.nn.parallel import DistributedDataParallel as DDP
        dev_ids = [device.index] if device.type == "cuda" else None
        # the MedNeXt trunk carries an unused `dummy_tensor` parameter (trainer.py:241-253 uses the same flag).
        # DDP wraps the NETWORK, not the whole module: the loss -- and with adaptive loss balancing the weighter's own parameters
        # (log-variances / task weights) -- is computed after the wrapped forward returns, where DDP's reducer would first mark those
        # parameters unused and then see their gradient hooks fire ("Expected to mark a variable ready only once").  The
        # reference computes its loss inside the wrapped training_step (lightning/model.py:863-910); here the weighter's few gradients
        # are averaged over the ranks by hand below, which gives every rank the same update DDP would.
        net = DDP(module.model, device_ids=dev_ids, find_unused_parameters=True)
        if module.loss_weighter is not None:
            weighter_params = [p for p in module.loss_weighter.parameters() if p.requires_grad]
    opt, sched = module.configure_optimizers()
    module._scheduler = sched
    resumed = module.restore_training_state(opt, sched)
    sc = getattr(cfg.optimization, "scheduler", None)
    interval = str(getattr(sc, "interval", "epoch") or "epoch").lower()
    frequency = max(1, int(getattr(sc, "frequency", 1) or 1))
    if interval not in ("epoch", "step"):
        raise ValueError(f"optimization.scheduler.interval must be 'epoch' or 'step', got {interval!r}")
    per_epoch = int(steps_per_epoch) if steps_per_epoch else max_steps
    plateau = isinstance(sched, torch.optim.lr_scheduler.ReduceLROnPlateau)
    clip = float(getattr(cfg.optimization, "gradient_clip_val", 0.0) or 0.0)
    accum = max(1, int(getattr(cfg.optimization, "accumulate_grad_batches", 1) or 1))
    history = []
    it = iter(batches)
    first = module.global_step if resumed else 0
    epoch_loss, epoch_n = 0.0, 0
    for step in range(first, max_steps):
        opt.zero_grad(set_to_none=True)
        for _ in range(accum):
            batch = {k: v.to(device, non_blocking=True) for k, v in next(it).items()}
            out = net(batch["image"])
            loss, logs = module._compute_loss(out, batch["label"], batch.get("mask"), batch.get("label_mask"))
            (loss / accum).backward()
        if weighter_params:
            world = torch.distributed.get_world_size()
            flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in weighter_params])
            torch.distributed.all_reduce(flat)
            at = 0
            for p in weighter_params:
                p.grad = (flat[at:at + p.numel()] / world).view_as(p).clone()
                at += p.numel()
        if clip > 0 and not hasattr(opt, "max_grad_norm"):     # FusedAdamW clips inside its update kernel
            # every parameter the optimizer owns (with a loss weighter: its parameters too), as Lightning clips (and as FusedAdamW does)
            torch.nn.utils.clip_grad_norm_([p for g in opt.param_groups for p in g["params"]], clip)
        opt.step()
        module.global_step = step + 1
        history.append(float(loss.detach()))
        epoch_loss, epoch_n = epoch_loss + history[-1], epoch_n + 1
        end_of_epoch = (step + 1) % per_epoch == 0
        if end_of_epoch:
            module.current_epoch += 1
        if sched is not None:
            if interval == "step":
                if (step + 1) % frequency == 0:
                    sched.step(history[-1]) if plateau else sched.step()
            elif end_of_epoch and module.current_epoch % frequency == 0:
                sched.step(epoch_loss / max(1, epoch_n)) if plateau else sched.step()
        if end_of_epoch:
            epoch_loss, epoch_n = 0.0, 0
        if step - first == 2:
            from ..utils.hostgc import quiesce_gc
            quiesce_gc()       # the cyclic GC's full passes cost milliseconds per step in a launch-bound loop
        if not math.isfinite(history[-1]):
            raise FloatingPointError(f"training loss is not finite at step {step}")
        if log and (step % log_every == 0 or step == max_steps - 1):
            log(f"step {step}: loss {history[-1]:.4f} lr {opt.param_groups[0]['lr']:.2e}")
        if val_batches is not None and val_every and ((step + 1) % int(val_every) == 0 or step == max_steps - 1):
            result = {"step": step + 1, **validate(module, val_batches, device=device)}
            module.val_history.append(result)
            if log:
                log("validation " + " ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in result.items()))
    return history, opt


def synthetic_batches(batch_size: int, patch, *, in_channels=1, out_channels=1, seed=42, device="cpu"):
    """The reference's random demo data (data_factory.py:273-276): image U[0,1), label rand > 0.85."""
    g = torch.Generator(device=device).manual_seed(seed)
    g2 = torch.Generator(device=device).manual_seed(seed + 1000)
    while True:
        img = torch.rand((batch_size, in_channels, *patch), generator=g, device=device)
        lab = (torch.rand((batch_size, out_channels, *patch), generator=g2, device=device) > 0.85).float()
        yield {"image": img, "label": lab}


__all__ = ["ConnectomicsModule", "build_optimizer", "build_lr_scheduler", "WarmupCosineLR", "fit", "validate", "resolve_training_steps",
           "match_target_to_output", "synthetic_batches", "check_label_mask", "resize_label_mask_to_output",
           "dice_loss_sigmoid", "weighted_bce_with_logits", "precision_to_dtype"]

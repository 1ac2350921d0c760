"""One row per loss name: everything ConnectomicsModule needs to know about a loss (the counterpart of the reference's
models/losses/metadata.py and build.py, laid out for this module's term plan).

A row's `build(**kwargs)` runs once, when the module is built: it checks the term's kwargs and returns what `_term_loss` calls on every
step.  Every `pred_target` loss is called as `loss(pred, target, spatial, fill=, pos_weight=)`; a `pred_only` / `pred_pred` loss is its
nn.Module, called on one or two prediction slices (and `mask=`).

Adding a loss: one row here, its kernels under csrc/ with their wrappers in hip_ops.py, and its cases under tests/.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import partial
from typing import Callable, Optional

import torch.nn.functional as F

from . import regularization_autograd as reg
from . import softmax_loss_autograd as sm
from .cldice_autograd import SoftClDiceLoss
from .losses import (_mask_for_unweighted_loss, monai_dice_loss, monai_focal_loss, monai_tversky_loss, per_channel_bce_with_logits,
                     weighted_bce_with_logits, weighted_regression_loss)
from .scnp_autograd import ScnpLoss


@dataclass(frozen=True)
class LossRow:
    build: Callable[..., Callable]      # (**the term's kwargs) -> the callable of the term; raises on kwargs the loss refuses
    call: str = "pred_target"           # or "pred_only" / "pred_pred": no target, one / two prediction slices (metadata.py:53-76)
    # the spatial argument: "weight" = a weight map (metadata.py:38-48); "mask" = a `mask` keyword; None = the term's mask goes by
    # position with `fill` and reaches the loss through its inputs (logits at the clamp minimum, target 0 outside it), or nowhere
    spatial: Optional[str] = None
    # "weight" rows only.  balance_map: the loss gets the class-balancing map when the term has no mask of its own; without it the
    # term's pos_weight reaches the loss itself, as a scalar.  own_pos_weight: the loss balances the classes by itself, so the term's
    # pos_weight defaults to 1 (plan.py:105-112)
    balance_map: bool = True
    own_pos_weight: bool = False
    target: str = "dense"               # or "class_index": one channel of labels, resized by nearest neighbour on every scale
    fused: Optional[str] = None         # "bce" / "dice": the term's share of the fused BCE + Dice reduction (training/fused.py)
    # a term judged apart from the fused reduction: it never enters it, and its presence does not push the other terms off it
    beside_fused: bool = False


def _regression(kind: str):
    def build(tanh=False, beta=1.0, **_unused):
        def loss(p, t, weight=None, *, fill=-20.0, pos_weight=None):
            return weighted_regression_loss(kind, p, t, weight, tanh=bool(tanh), beta=float(beta))
        return loss
    return build


def _weighted_bce(**_unused):
    def loss(p, t, weight=None, *, fill=-20.0, pos_weight=None):
        return weighted_bce_with_logits(p, t, weight, pos_weight)
    return loss


def _per_channel_bce(auto_pos_weight=True, max_pos_weight=10.0, reduction="mean", **_unused):
    def loss(p, t, weight=None, *, fill=-20.0, pos_weight=None):
        return per_channel_bce_with_logits(p, t, weight, auto_pos_weight=bool(auto_pos_weight), max_pos_weight=float(max_pos_weight),
                                           reduction=str(reduction))
    return loss


def _weighted_module(cls):
    """A loss class called as module(pred, target, weight=): built once per term, so its argument checks run with the module's."""
    def build(**kwargs):
        module = cls(**kwargs)

        def loss(p, t, weight=None, *, fill=-20.0, pos_weight=None):
            v = module(p, t, weight=weight)
            # `reduction: none` leaves a per-(sample, channel) tensor, which the reference's orchestrator cannot take as a term unless
            # it holds one value (its finiteness check and `.item()` fail otherwise); the same case is refused here by name
            if v.numel() != 1:
                raise ValueError(f"{cls.__name__} with reduction='none' returned a loss of shape {tuple(v.shape)}: a training loss "
                                 "term must reduce to one value (use reduction 'mean' or 'sum')")
            return v
        return loss
    return build


def _through_inputs(fn):
    """A loss without a spatial argument (MONAI's and torch's own): the mask reaches it as a masked_fill copy of its inputs."""
    def build(**kwargs):
        def loss(p, t, mask=None, *, fill=-20.0, pos_weight=None):
            return fn(*_mask_for_unweighted_loss(p, t, mask, fill), **kwargs)
        return loss
    return build


def _torch_mean(fn):
    return lambda p, t, **_unused: fn(p.float(), t.float())


def _by_position(fn, check):
    """The softmax losses and L1Loss: called as fn(pred, target, mask, fill=, **kwargs) -- `weight` in the kwargs is the CLASS weight of
    CrossEntropyLoss / DiceCELoss --, so the HIP kernels see the mask itself, never a masked_fill copy of the logits."""
    def build(**kwargs):
        check(**kwargs)

        def loss(p, t, mask=None, *, fill=-20.0, pos_weight=None):
            return fn(p, t, mask, fill=fill, **kwargs)
        return loss
    return build


LOSS_TABLE = {
    "WeightedMSELoss": LossRow(_regression("mse"), spatial="weight"),
    "WeightedMAELoss": LossRow(_regression("mae"), spatial="weight"),
    "SmoothL1Loss": LossRow(_regression("huber"), spatial="weight"),
    "WeightedBCEWithLogitsLoss": LossRow(_weighted_bce, spatial="weight", balance_map=False, own_pos_weight=True, fused="bce"),
    "PerChannelBCEWithLogitsLoss": LossRow(_per_channel_bce, spatial="weight", own_pos_weight=True),
    # topology loss (losses.py:456-721): soft skeletons on HIP for CUDA tensors (training/cldice_autograd.py)
    "SoftClDiceLoss": LossRow(_weighted_module(SoftClDiceLoss), spatial="weight"),
    # neighbour-penalised per-channel BCE (losses.py:354-453): pooled logits, sums and gradient on HIP (training/scnp_autograd.py)
    "ScnpLoss": LossRow(_weighted_module(ScnpLoss), spatial="weight"),
    "DiceLoss": LossRow(_through_inputs(monai_dice_loss), fused="dice"),           # the sigmoid / plain form; see loss_row
    "TverskyLoss": LossRow(_through_inputs(monai_tversky_loss)),
    "FocalLoss": LossRow(_through_inputs(monai_focal_loss)),
    "BCEWithLogitsLoss": LossRow(_through_inputs(_torch_mean(F.binary_cross_entropy_with_logits)), fused="bce"),
    "MSELoss": LossRow(_through_inputs(_torch_mean(F.mse_loss))),
    # the regularisers (models/losses/regularization.py; value and gradients on HIP, training/regularization_autograd.py)
    "BinaryRegularization": LossRow(reg.BinaryRegularization, beside_fused=True, call="pred_only", spatial="mask"),
    "NonOverlapRegularization": LossRow(reg.NonOverlapRegularization, beside_fused=True, call="pred_only"),
    "ForegroundDistanceConsistency": LossRow(reg.ForegroundDistanceConsistency, beside_fused=True, call="pred_pred", spatial="mask"),
    "ContourDistanceConsistency": LossRow(reg.ContourDistanceConsistency, beside_fused=True, call="pred_pred", spatial="mask"),
    "ForegroundContourConsistency": LossRow(reg.ForegroundContourConsistency, beside_fused=True, call="pred_pred", spatial="mask"),
    # the softmax losses and L1Loss (training/softmax_loss_autograd.py)
    "CrossEntropyLoss": LossRow(_by_position(sm.cross_entropy_loss, sm.check_cross_entropy_kwargs), target="class_index", beside_fused=True),
    "DiceCELoss": LossRow(_by_position(sm.dice_ce_loss, sm.check_dice_ce_kwargs), beside_fused=True),
    "GeneralizedDiceLoss": LossRow(_by_position(sm.generalized_dice_loss, sm.check_generalized_dice_kwargs), beside_fused=True),
    "L1Loss": LossRow(_by_position(sm.l1_loss, sm.check_l1_kwargs), beside_fused=True),
}
_SOFTMAX_DICE = LossRow(_by_position(sm.softmax_dice_loss, partial(sm.check_softmax_dice_kwargs, "DiceLoss")), beside_fused=True)


def loss_row(fn: str, kwargs) -> LossRow:
    """The row of a term.  A DiceLoss term takes the softmax path only when `softmax` or `to_onehot_y` is set; the sigmoid / plain form
    keeps its own."""
    if fn not in LOSS_TABLE:
        raise ValueError(f"Unknown loss function {fn!r}; available: {sorted(LOSS_TABLE)}")
    if fn == "DiceLoss" and bool(kwargs.get("softmax", False) or kwargs.get("to_onehot_y", False)):
        return _SOFTMAX_DICE
    return LOSS_TABLE[fn]


__all__ = ["LossRow", "LOSS_TABLE", "loss_row"]

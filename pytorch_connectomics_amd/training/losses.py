"""The loss functions that are plain torch ops on the device, and the helpers the loss terms of ConnectomicsModule share: MONAI's
Dice / Tversky / Focal restated, the weighted and per-channel BCE, the weighted regression losses, the class-balancing weight map and
the "mask through the inputs" rule.  The losses with HIP kernels of their own live in the *_autograd modules; training/loss_table.py
says how the module calls each of them."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F


def dice_loss_sigmoid(logits: torch.Tensor, target: torch.Tensor, smooth_nr: float = 1e-5, smooth_dr: float = 1e-5):
    """MONAI DiceLoss(sigmoid=True) semantics: per (B, C) dice over spatial dims, mean over B and C."""
    p = torch.sigmoid(logits.float())
    t = target.float()
    dims = tuple(range(2, p.dim()))
    inter = (p * t).sum(dims)
    den = p.sum(dims) + t.sum(dims)
    return (1.0 - (2.0 * inter + smooth_nr) / (den + smooth_dr)).mean()


def _mask_for_unweighted_loss(pred, target, mask, clamp_min: float):
    """Losses without a spatial-weight argument (the MONAI ones) see a mask through their INPUTS
    (training/losses/orchestrator.py:648-655): invalid voxels get the clamp floor as logit and 0 as target."""
    if mask is None:
        return pred, target
    valid = (mask > 0).expand_as(pred)
    return pred.masked_fill(~valid, float(clamp_min)), target * (mask > 0).to(target.dtype)


def _drop_background(p, t, include_background: bool):
    if include_background or p.shape[1] == 1:          # MONAI: "single channel prediction, include_background=False ignored"
        return p, t
    return p[:, 1:], t[:, 1:]


def monai_dice_loss(logits, target, *, sigmoid: bool = False, include_background: bool = True, smooth_nr=1e-5, smooth_dr=1e-5,
                    squared_pred: bool = False, **_unused):
    """monai.losses.DiceLoss as the reference instantiates it (models/losses/build.py:58-61; reduction 'mean', batch=False):
    1 - (2 sum(p t) + smooth_nr) / (sum(p) + sum(t) + smooth_dr) per (B, C) over the spatial dims, mean over B and C.
    `sigmoid` defaults to False as in MONAI (a config that omits it trains Dice on the raw logits).  Parity unpinned: MONAI
    is not in the image; restated from its documented formula."""
    p = torch.sigmoid(logits.float()) if sigmoid else logits.float()
    t = target.float()
    p, t = _drop_background(p, t, bool(include_background))
    dims = tuple(range(2, p.dim()))
    inter = (p * t).sum(dims)
    den = ((p * p).sum(dims) + (t * t).sum(dims)) if squared_pred else (p.sum(dims) + t.sum(dims))
    return (1.0 - (2.0 * inter + float(smooth_nr)) / (den + float(smooth_dr))).mean()


def monai_tversky_loss(logits, target, *, sigmoid: bool = False, include_background: bool = True, alpha: float = 0.5,
                       beta: float = 0.5, smooth_nr=1e-5, smooth_dr=1e-5, **_unused):
    """monai.losses.TverskyLoss: tp = sum(p t), fp = alpha sum(p (1 - t)), fn = beta sum((1 - p) t) per (B, C);
    1 - (tp + smooth_nr) / (tp + fp + fn + smooth_dr), mean.  Parity unpinned (see monai_dice_loss)."""
    p = torch.sigmoid(logits.float()) if sigmoid else logits.float()
    t = target.float()
    p, t = _drop_background(p, t, bool(include_background))
    dims = tuple(range(2, p.dim()))
    tp = (p * t).sum(dims)
    fp = float(alpha) * (p * (1.0 - t)).sum(dims)
    fn = float(beta) * ((1.0 - p) * t).sum(dims)
    return (1.0 - (tp + float(smooth_nr)) / (tp + fp + fn + float(smooth_dr))).mean()


def monai_focal_loss(logits, target, *, gamma: float = 2.0, alpha=None, include_background: bool = True, **_unused):
    """monai.losses.FocalLoss (sigmoid form, use_softmax=False, reduction 'mean'): BCE-with-logits * (1 - p_t)^gamma, with
    alpha: * (alpha t + (1 - alpha)(1 - t)); mean over every element.  Parity unpinned (see monai_dice_loss)."""
    x, t = logits.float(), target.float()
    x, t = _drop_background(x, t, bool(include_background))
    bce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
    # (1 - p_t)^gamma = exp(gamma * logsigmoid(-x (2t - 1))): stable for large |x|
    mod = torch.exp(float(gamma) * F.logsigmoid(-x * (2.0 * t - 1.0)))
    loss = mod * bce
    if alpha is not None:
        loss = loss * (float(alpha) * t + (1.0 - float(alpha)) * (1.0 - t))
    return loss.mean()


def auto_pos_weight_scalar(target, mask=None, cap: float = 10.0) -> torch.Tensor:
    """`pos_weight: auto` of a weighted-BCE term (orchestrator.py:180-197): min(neg / pos, 10) over the valid voxels, 1 when
    either class is absent -- computed on the device, no host synchronisation."""
    valid = torch.ones_like(target, dtype=torch.bool) if mask is None else (mask > 0).expand_as(target)
    pos = ((target > 0) & valid).sum().float()
    neg = ((target <= 0) & valid).sum().float()
    ratio = torch.clamp(neg / pos.clamp_min(1.0), max=float(cap))
    return torch.where((pos > 0) & (neg > 0), ratio, torch.ones_like(ratio)).reshape(1)


def class_balance_weight(target: torch.Tensor, pos_weight=None, valid_mask=None, cap: float = 10.0) -> torch.Tensor:
    """The spatial weight map the reference's orchestrator hands to every `weight`-taking loss except the weighted BCE when a term
    carries no mask of its own (orchestrator.py:129-178, :606-612).  `pos_weight` None / "auto": foreground (target > 0) and
    background weights in the ratio neg : pos, scaled so that the valid voxels average 1, each capped at `cap`; ones when a class
    is absent.  A number: that weight on the foreground, 1 elsewhere.  Counts stay on the device (no host synchronisation)."""
    t = target
    ones = torch.ones_like(t)
    if pos_weight is not None and not isinstance(pos_weight, str):
        fg = float(pos_weight)
        if fg <= 0:
            raise ValueError(f"pos_weight must be > 0, got {fg}")
        return torch.where(t > 0, ones * fg, ones)
    if isinstance(pos_weight, str) and pos_weight != "auto":
        raise ValueError(f"Unsupported pos_weight mode: {pos_weight!r}. Expected a positive number or 'auto'.")
    valid = torch.ones_like(t, dtype=torch.bool) if valid_mask is None else (valid_mask > 0).expand_as(t)
    pos = ((t > 0) & valid).sum().to(t.dtype if t.is_floating_point() else torch.float32)
    neg = ((t <= 0) & valid).sum().to(pos.dtype)
    both = (pos > 0) & (neg > 0)
    count = pos + neg
    fg = torch.clamp(count / (2.0 * pos.clamp_min(1.0)), max=float(cap))
    bg = torch.clamp(count / (2.0 * neg.clamp_min(1.0)), max=float(cap))
    balanced = torch.where(t > 0, ones * fg, ones * bg)
    return torch.where(both, balanced, ones)


def per_channel_bce_with_logits(logits, target, weight=None, *, auto_pos_weight: bool = True, max_pos_weight: float = 10.0,
                                reduction: str = "mean"):
    """models/losses/losses.py:269-351: BCE per channel with its own class-balancing weight min(n_neg / n_pos, max_pos_weight)
    (1 for a channel without positives) from the valid voxels of the current batch, reduced per channel (weighted-valid mean or
    sum), summed over the channels."""
    x, t = logits.float(), target.float()
    C = x.shape[1]
    pw = None
    if auto_pos_weight:
        valid = (weight > 0).expand_as(t) if weight is not None else torch.ones_like(t, dtype=torch.bool)
        dims = (0,) + tuple(range(2, t.dim()))
        pos = ((t > 0) & valid).sum(dims).float()
        neg = ((t <= 0) & valid).sum(dims).float()
        ratio = torch.clamp(neg / pos.clamp_min(1.0), max=float(max_pos_weight))
        pw = torch.where(pos > 0, ratio, torch.ones_like(ratio)).reshape(1, C, *([1] * (t.dim() - 2)))
    bce = F.binary_cross_entropy_with_logits(x, t, pos_weight=pw, reduction="none")
    total = x.new_zeros(())
    w = None if weight is None else weight.float().expand_as(bce)
    for c in range(C):
        b = bce[:, c:c + 1]
        if w is None:
            total = total + (b.mean() if reduction == "mean" else b.sum())
        else:
            wc = w[:, c:c + 1]
            bw = b * wc
            valid_c = wc > 0
            total = total + ((bw * valid_c).sum() / valid_c.sum().clamp_min(1) if reduction == "mean" else bw.sum())
    return total


def weighted_bce_with_logits(logits, target, weight=None, pos_weight=None):
    """models/losses/losses.py:17-44,190-266 (reduction='mean'; with a weight map: the mean of weight * bce over the
    voxels whose weight is > 0, the map broadcast to the logits' shape; 0 when no voxel is valid)."""
    if pos_weight is None:
        pw = None
    elif isinstance(pos_weight, str):
        if pos_weight != "auto":
            raise ValueError(f"Unsupported pos_weight mode: {pos_weight!r}. Expected a positive number or 'auto'.")
        pw = auto_pos_weight_scalar(target, weight).to(logits.device)
    elif isinstance(pos_weight, torch.Tensor):
        pw = pos_weight.to(device=logits.device, dtype=torch.float32)
    else:
        if float(pos_weight) <= 0:
            raise ValueError(f"pos_weight must be > 0, got {float(pos_weight)}")
        pw = torch.as_tensor([float(pos_weight)], device=logits.device, dtype=torch.float32)
    bce = F.binary_cross_entropy_with_logits(logits.float(), target.float(), pos_weight=pw, reduction="none")
    if weight is None:
        return bce.mean()
    w = weight.float().expand_as(bce)
    valid = w > 0
    return (bce * w * valid).sum() / valid.sum().clamp_min(1)


def _reduce_weighted(loss: torch.Tensor, weight: Optional[torch.Tensor]) -> torch.Tensor:
    """losses.py:17-44 with reduction='mean': plain mean, or the mean of weight * loss over the voxels with weight > 0."""
    if weight is None:
        return loss.mean()
    w = weight.float().expand_as(loss)
    valid = w > 0
    return (loss * w * valid).sum() / valid.sum().clamp_min(1)


def weighted_regression_loss(kind: str, pred, target, weight=None, *, tanh: bool = False, beta: float = 1.0):
    """WeightedMSELoss / WeightedMAELoss / SmoothL1Loss of the reference (losses.py:140-187, 725-800): optional tanh on
    the prediction (distance-transform targets in [-1, 1]), elementwise loss, weighted-valid mean."""
    p = pred.float()
    if tanh:
        p = torch.tanh(p)
    t = target.float()
    if kind == "mse":
        loss = (p - t) ** 2
    elif kind == "mae":
        loss = (p - t).abs()
    else:
        loss = F.smooth_l1_loss(p, t, beta=float(beta), reduction="none")
    return _reduce_weighted(loss, weight)

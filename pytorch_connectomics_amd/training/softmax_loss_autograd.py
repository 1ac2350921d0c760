"""The softmax (mutually exclusive class) losses: CrossEntropyLoss, DiceLoss(softmax / to_onehot_y), DiceCELoss and
GeneralizedDiceLoss, all finalised from one (N, C, 8) tensor of sums (csrc/softmax_loss_kernels.hip), plus the small L1Loss row.

`softmax_loss_sums` reduces the channel softmax p of the logits against the target t to, per (sample, class), the sums over voxels of

    0: p t    1: p    2: p^2    3: t    4: t^2    5: valid t (-logp)    6: valid (-logp)    7: valid t

CUDA tensors run the HIP kernel pair (one streaming read forward; one read and one write backward, the softmax recomputed; no copy
of the logits, no atomics, no host synchronisation); CPU tensors -- and CUDA tensors with `use_hip=False` -- run the torch
restatement `softmax_loss_sums_torch`, in the dtype they are given and for any C.  Everything loss-specific is torch on the sums.

Target forms, detected as the reference does: a target with a singleton channel, or one dimension fewer than the logits, is a class
index (t = onehot; a voxel whose label is `ignore_index` is CE-invalid and has t = 0); a target of the logits' shape is dense.  A label
outside [0, C) that is not `ignore_index` raises nothing on the device: column 5 of its sample becomes NaN, so the loss is not finite.

A mask reaches the losses "through the inputs" (reference training/losses/orchestrator.py:649-656): where mask <= 0 the logits read
as `fill` (the module's clamp minimum) and the target as 0 -- class 0 for an index target.  With a C-channel mask an index label reads
0 unless every channel of its voxel is valid (the reference defines no such case).

`CrossEntropyLoss` is pinned to the reference's CrossEntropyLossWrapper (tests/golden/softmax_losses.npz).  The three MONAI forms
are restated from MONAI's documented formulas: parity unpinned (MONAI is not installed where this was written).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from .hip_dispatch import channel_mask, wants_hip

SUM_COLUMNS = ("pt", "p", "pp", "t", "tt", "ce", "nlogp", "t_valid")


def target_form(logits: torch.Tensor, target: torch.Tensor):
    """-> ("dense", target) or ("index", labels of shape (N, *spatial)) as the reference's wrapper decides it (losses.py:126-135)."""
    if target.dim() == logits.dim() - 1 and target.shape == logits.shape[:1] + logits.shape[2:]:
        return "index", target
    if target.dim() == logits.dim() and target.shape[1] == 1 and logits.shape[1] != 1 and target.shape[2:] == logits.shape[2:] \
            and target.shape[0] == logits.shape[0]:
        return "index", target[:, 0]
    if target.shape == logits.shape:
        return "dense", target
    raise ValueError(f"target of shape {tuple(target.shape)} is neither dense {tuple(logits.shape)} nor a class index with a singleton "
                     "channel or without one")


def softmax_loss_sums_torch(logits, target, mask=None, *, ignore_index: int = -100, fill: float = -20.0):
    """The eight columns in plain torch, in the logits' dtype, for any C (the CPU path and the yardstick of the GPU tests)."""
    x = logits
    C = x.shape[1]
    form, tgt = target_form(x, target)
    mask = channel_mask(mask, x)
    live = None
    if mask is not None:
        live = (mask > 0).expand_as(x)
        x = torch.where(live, x, torch.full((), float(fill), dtype=x.dtype, device=x.device))
    bad_sample = None
    if form == "dense":
        t = tgt.to(x.dtype)
        if live is not None:
            t = t * live.to(x.dtype)
        valid = torch.ones_like(x[:, :1])
    else:
        y = tgt.long()
        if live is not None:
            y = y * live.all(dim=1).to(y.dtype)
        ignored = y == int(ignore_index)
        bad = ~ignored & ((y < 0) | (y >= C))
        keep = ~(ignored | bad)
        t = torch.movedim(F.one_hot(torch.where(keep, y, torch.zeros_like(y)), C), -1, 1).to(x.dtype) * keep.unsqueeze(1).to(x.dtype)
        valid = (~ignored).unsqueeze(1).to(x.dtype)
        bad_sample = bad.flatten(1).any(dim=1)
    nlogp = -F.log_softmax(x, dim=1)
    p = torch.exp(-nlogp)
    cols = [p * t, p, p * p, t, t * t, valid * (t * nlogp), valid * nlogp, valid * t]
    sums = torch.stack([c.expand_as(x).flatten(2).sum(-1) for c in cols], dim=-1)
    if bad_sample is not None:
        poison = torch.zeros_like(sums)
        poison[..., 5] = float("nan")
        sums = torch.where(bad_sample.view(-1, 1, 1), sums + poison, sums)
    return sums


class SoftmaxLossSumsFn(torch.autograd.Function):
    """(logits, target, mask or None, ignore_index, fill) -> sums (N, C, 8); saves the operands only."""

    @staticmethod
    def forward(ctx, logits, target, mask, ignore_index: int, fill: float):
        from .. import hip_ops as ops
        sums = ops.softmax_loss_forward(logits, target, mask, ignore_index=ignore_index, fill=fill)
        ctx.save_for_backward(logits, target, mask)
        ctx.ignore_index, ctx.fill = int(ignore_index), float(fill)
        return sums

    @staticmethod
    def backward(ctx, gsums):
        from .. import hip_ops as ops
        logits, target, mask = ctx.saved_tensors
        dx = ops.softmax_loss_backward(gsums, logits, target, mask, ignore_index=ctx.ignore_index, fill=ctx.fill)
        return dx, None, None, None, None


def softmax_loss_sums(logits, target, mask=None, *, ignore_index: int = -100, fill: float = -20.0, use_hip: Optional[bool] = None):
    """-> (N, C, 8) sums (see the module docstring), differentiable in the logits."""
    if logits.dim() < 3:
        raise ValueError(f"softmax losses expect (N, C, *spatial) logits, got {tuple(logits.shape)}")
    if not wants_hip(use_hip, logits, "softmax_loss_sums"):
        return softmax_loss_sums_torch(logits, target, mask, ignore_index=ignore_index, fill=fill)
    C = int(logits.shape[1])
    if not 2 <= C <= 32:
        raise NotImplementedError(f"the softmax-loss kernels cover 2 <= C <= 32 classes, got C = {C} (CPU tensors, or use_hip=False, "
                                  "take any C)")
    form, tgt = target_form(logits, target)
    tgt = tgt.detach()
    if form == "dense" or tgt.dtype.is_floating_point:
        tgt = tgt.float()
    elif tgt.dtype != torch.int64:
        tgt = tgt.long()
    if mask is not None:
        mask = channel_mask(mask.detach().float(), logits)          # in its own layout: the kernels take strides
    return SoftmaxLossSumsFn.apply(logits.float(), tgt, mask, int(ignore_index), float(fill))


# ---- finalisers: torch on the (N, C, 8) sums, no host synchronisation ----------------------------------------------------------------
def _check_reduction(name: str, reduction: str, allowed=("mean", "sum")):
    if reduction not in allowed:
        raise ValueError(f"{name} reduction must be {' or '.join(repr(a) for a in allowed)}, got {reduction!r}: a training loss term "
                         "must reduce to a scalar")


def check_cross_entropy_kwargs(weight=None, ignore_index: int = -100, reduction: str = "mean", label_smoothing: float = 0.0,
                               use_hip: Optional[bool] = None):
    _check_reduction("CrossEntropyLoss", reduction)
    if not 0.0 <= float(label_smoothing) <= 1.0:
        raise ValueError(f"label_smoothing must be between 0.0 and 1.0. Got: {float(label_smoothing)}")           # torch's words


def _ce_from_sums(S, form: str, voxels: int, *, weight, reduction: str, label_smoothing: float):
    C = S.shape[1]
    eps = float(label_smoothing)
    if weight is None:
        w = torch.ones((C,), dtype=S.dtype, device=S.device)
    else:
        w = torch.as_tensor(weight, dtype=S.dtype, device=S.device).reshape(-1)
        if w.numel() != C:
            raise ValueError("weight tensor should be defined either for all or no classes")                          # torch's words
    num = (w * ((1.0 - eps) * S[..., 5] + (eps / C) * S[..., 6])).sum()
    if reduction == "sum":
        return num
    if form == "dense":
        return num / float(voxels)
    return num / (w * S[..., 7]).sum()


def cross_entropy_loss(logits, target, mask=None, *, fill: float = -20.0, weight=None, ignore_index: int = -100, reduction: str = "mean",
                       label_smoothing: float = 0.0, use_hip: Optional[bool] = None):
    """The reference's CrossEntropyLossWrapper (models/losses/losses.py:88-137) over nn.CrossEntropyLoss.  Index targets: sum_c w_c
    [(1 - eps) S5_c + (eps / C) S6_c], divided by sum_c w_c S7_c for 'mean'; dense (probability) targets divide by the voxel count."""
    check_cross_entropy_kwargs(weight, ignore_index, reduction, label_smoothing)
    form, _ = target_form(logits, target)
    S = softmax_loss_sums(logits, target, mask, ignore_index=ignore_index, fill=fill, use_hip=use_hip)
    return _ce_from_sums(S, form, logits.numel() // logits.shape[1], weight=weight, reduction=reduction,
                         label_smoothing=label_smoothing)


def check_softmax_dice_kwargs(name: str = "DiceLoss", *, include_background: bool = True, to_onehot_y: bool = False, sigmoid: bool = False,
                              softmax: bool = False, other_act=None, squared_pred: bool = False, jaccard: bool = False,
                              reduction: str = "mean", smooth_nr: float = 1e-5, smooth_dr: float = 1e-5, batch: bool = False, weight=None,
                              use_hip: Optional[bool] = None):
    if softmax and sigmoid:
        raise ValueError(f"{name}: softmax=True together with sigmoid=True; choose one activation")
    if other_act is not None:
        raise NotImplementedError(f"{name} other_act is not built")
    if batch:
        raise NotImplementedError(f"{name} batch=True is not built")
    if weight is not None and name == "DiceLoss":
        raise NotImplementedError(f"{name} weight is not built")
    if reduction != "mean":
        raise NotImplementedError(f"{name} reduction={reduction!r} is not built: only 'mean'")


def _dice_from_sums(S, *, include_background: bool, squared_pred: bool, jaccard: bool, smooth_nr: float, smooth_dr: float):
    if not include_background and S.shape[1] > 1:
        S = S[:, 1:]
    inter = S[..., 0]
    den = (S[..., 2] + S[..., 4]) if squared_pred else (S[..., 1] + S[..., 3])
    if jaccard:
        den = 2.0 * (den - inter)
    # (column 5 enters with weight 0: it is NaN where a label was out of range, and so is the loss then, as for the CE forms)
    return (1.0 - (2.0 * inter + float(smooth_nr)) / (den + float(smooth_dr))).mean() + 0.0 * S[..., 5].sum()


def softmax_dice_loss(logits, target, mask=None, *, fill: float = -20.0, include_background: bool = True, to_onehot_y: bool = False,
                      sigmoid: bool = False, softmax: bool = False, squared_pred: bool = False, jaccard: bool = False,
                      smooth_nr: float = 1e-5, smooth_dr: float = 1e-5, use_hip: Optional[bool] = None, **rest):
    """monai.losses.DiceLoss with `softmax=True` and / or `to_onehot_y=True` (reduction 'mean', batch=False): 1 - (2 sum(p t) +
    smooth_nr) / (sum(p) + sum(t) + smooth_dr) per (sample, class) -- p^2 and t^2 with squared_pred; the denominator 2 (den - sum(p t))
    with jaccard --, mean over samples and classes.  With softmax the sums come from the HIP kernels; `to_onehot_y` without softmax
    scores sigmoid(x) or the raw logits against the one-hot target with torch ops (F.one_hot, torch.where) on CUDA tensors too: no
    softmax, so no kernel.  There a label outside [0, C) makes the loss NaN, as on the kernel path (this form has no ignore_index).
    Parity unpinned: restated from MONAI's documented formula."""
    check_softmax_dice_kwargs("DiceLoss", include_background=include_background, to_onehot_y=to_onehot_y, sigmoid=sigmoid, softmax=softmax,
                              squared_pred=squared_pred, jaccard=jaccard, smooth_nr=smooth_nr, smooth_dr=smooth_dr, **rest)
    form, tgt = target_form(logits, target)
    if form == "index" and not to_onehot_y:
        raise ValueError("DiceLoss: a class-index target needs to_onehot_y=True")
    if form == "dense" and to_onehot_y:
        raise ValueError("DiceLoss: to_onehot_y=True needs a class-index target with one channel")
    if softmax:
        S = softmax_loss_sums(logits, target, mask, fill=fill, use_hip=use_hip)
    else:
        x = logits
        C = x.shape[1]
        m = channel_mask(mask, x)
        y = tgt.long()
        if m is not None:
            live = (m > 0).expand_as(x)
            x = torch.where(live, x, torch.full((), float(fill), dtype=x.dtype, device=x.device))
            y = y * live.all(dim=1).to(y.dtype)
        p = torch.sigmoid(x) if sigmoid else x
        bad = (y < 0) | (y >= C)                              # no ignore_index here: the NaN rule of the sums, on every column
        t = torch.movedim(F.one_hot(y.clamp(0, C - 1), C), -1, 1).to(p.dtype)
        z = torch.zeros_like(p)
        S = torch.stack([c.flatten(2).sum(-1) for c in (p * t, p, p * p, t, t * t, z, z, z)], dim=-1)
        S = torch.where(bad.flatten(1).any(dim=1).view(-1, 1, 1), torch.full_like(S, float("nan")), S)
    return _dice_from_sums(S, include_background=include_background, squared_pred=squared_pred, jaccard=jaccard, smooth_nr=smooth_nr,
                           smooth_dr=smooth_dr)


def check_dice_ce_kwargs(*, include_background: bool = True, to_onehot_y: bool = False, sigmoid: bool = False, softmax: bool = False,
                         other_act=None, squared_pred: bool = False, jaccard: bool = False, reduction: str = "mean",
                         smooth_nr: float = 1e-5, smooth_dr: float = 1e-5, batch: bool = False, weight=None, lambda_dice: float = 1.0,
                         lambda_ce: float = 1.0, label_smoothing: float = 0.0, use_hip: Optional[bool] = None):
    check_softmax_dice_kwargs("DiceCELoss", sigmoid=sigmoid, softmax=softmax, other_act=other_act, reduction=reduction, batch=batch)
    if not softmax:
        raise NotImplementedError("DiceCELoss is built in its softmax=True form only")
    if float(lambda_dice) < 0.0:
        raise ValueError("lambda_dice should be no less than 0.0.")
    if float(lambda_ce) < 0.0:
        raise ValueError("lambda_ce should be no less than 0.0.")


def dice_ce_loss(logits, target, mask=None, *, fill: float = -20.0, use_hip: Optional[bool] = None, **kw):
    """monai.losses.DiceCELoss, softmax form: lambda_dice x the softmax Dice + lambda_ce x the cross entropy, both from ONE pass over
    the logits.  MONAI's arguments and defaults; `weight` is the CE class weight.  With to_onehot_y=True the CE half sees the index
    target and the Dice half its one-hot form; a dense target enters the CE half as class probabilities.  A one-channel prediction
    (MONAI's BCE branch) is refused.  Deviation: `weight` reaches the CE half only; current MONAI also weights the Dice half's
    classes with it.  Parity unpinned: restated from MONAI's documented formula."""
    check_dice_ce_kwargs(**kw)
    if logits.shape[1] == 1:
        raise NotImplementedError("DiceCELoss on a one-channel prediction (MONAI's BCE branch) is not built")
    form, _ = target_form(logits, target)
    onehot = bool(kw.get("to_onehot_y", False))
    if form == "index" and not onehot:
        raise ValueError("DiceCELoss: a class-index target needs to_onehot_y=True")
    if form == "dense" and onehot:
        raise ValueError("DiceCELoss: to_onehot_y=True needs a class-index target with one channel")
    S = softmax_loss_sums(logits, target, mask, fill=fill, use_hip=use_hip)
    dice = _dice_from_sums(S, include_background=bool(kw.get("include_background", True)), squared_pred=bool(kw.get("squared_pred", False)),
                           jaccard=bool(kw.get("jaccard", False)), smooth_nr=kw.get("smooth_nr", 1e-5), smooth_dr=kw.get("smooth_dr", 1e-5))
    ce = _ce_from_sums(S, form, logits.numel() // logits.shape[1], weight=kw.get("weight"), reduction="mean",
                       label_smoothing=float(kw.get("label_smoothing", 0.0)))
    return float(kw.get("lambda_dice", 1.0)) * dice + float(kw.get("lambda_ce", 1.0)) * ce


def check_generalized_dice_kwargs(*, include_background: bool = True, to_onehot_y: bool = False, sigmoid: bool = False,
                                  softmax: bool = False, other_act=None, w_type: str = "square", reduction: str = "mean",
                                  smooth_nr: float = 1e-5, smooth_dr: float = 1e-5, batch: bool = False,
                                  use_hip: Optional[bool] = None):
    check_softmax_dice_kwargs("GeneralizedDiceLoss", sigmoid=sigmoid, softmax=softmax, other_act=other_act, reduction=reduction, batch=batch)
    if not softmax:
        raise NotImplementedError("GeneralizedDiceLoss is built in its softmax=True form only")
    if str(w_type) not in ("square", "simple", "uniform"):
        raise ValueError(f"GeneralizedDiceLoss w_type must be 'square', 'simple' or 'uniform', got {w_type!r}")


def generalized_dice_loss(logits, target, mask=None, *, fill: float = -20.0, use_hip: Optional[bool] = None, **kw):
    """monai.losses.GeneralizedDiceLoss, softmax form: class weights w = 1 / S3^2 ('square'), 1 / S3 ('simple') or 1 ('uniform'), an
    infinite weight replaced by the largest finite weight of its sample; 1 - (2 sum_c w S0 + smooth_nr) / (sum_c w (S1 + S3) +
    smooth_dr) per sample, mean over samples.  Parity unpinned: restated from MONAI's documented formula."""
    check_generalized_dice_kwargs(**kw)
    form, _ = target_form(logits, target)
    onehot = bool(kw.get("to_onehot_y", False))
    if form == "index" and not onehot:
        raise ValueError("GeneralizedDiceLoss: a class-index target needs to_onehot_y=True")
    if form == "dense" and onehot:
        raise ValueError("GeneralizedDiceLoss: to_onehot_y=True needs a class-index target with one channel")
    S = softmax_loss_sums(logits, target, mask, fill=fill, use_hip=use_hip)
    if not bool(kw.get("include_background", True)) and S.shape[1] > 1:
        S = S[:, 1:]
    g = S[..., 3].detach()
    w_type = str(kw.get("w_type", "square"))
    w = torch.ones_like(g) if w_type == "uniform" else (1.0 / g if w_type == "simple" else 1.0 / (g * g))
    infs = torch.isinf(w)
    w = torch.where(infs, torch.zeros_like(w), w)
    w = w + infs.to(w.dtype) * w.max(dim=1, keepdim=True).values
    numer = 2.0 * (w * S[..., 0]).sum(1) + float(kw.get("smooth_nr", 1e-5))
    denom = (w * (S[..., 1] + S[..., 3])).sum(1) + float(kw.get("smooth_dr", 1e-5))
    return (1.0 - numer / denom).mean() + 0.0 * S[..., 5].sum()          # NaN where a label was out of range (see _dice_from_sums)


def check_l1_kwargs(reduction: str = "mean"):
    _check_reduction("L1Loss", reduction)


def l1_loss(pred, target, mask=None, *, fill: float = -20.0, reduction: str = "mean"):
    """torch's L1Loss with the mask through the inputs (the twin of the MSELoss row); no kernel."""
    check_l1_kwargs(reduction)
    p, t = pred.float(), target.float()
    if mask is not None:
        valid = (mask > 0).expand_as(p)
        p = p.masked_fill(~valid, float(fill))
        t = t * (mask > 0).to(t.dtype)
    return F.l1_loss(p, t, reduction=reduction)


__all__ = ["softmax_loss_sums", "softmax_loss_sums_torch", "target_form", "cross_entropy_loss", "softmax_dice_loss", "dice_ce_loss",
           "generalized_dice_loss", "l1_loss", "SUM_COLUMNS"]

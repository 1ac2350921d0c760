"""SoftClDiceLoss: the reference's topology loss (connectomics/models/losses/losses.py:47-85, :456-721) with the soft skeleton and its
gradient on HIP (csrc/cldice_kernels.hip).

CUDA tensors run the kernels: both skeletons, the four weighted sums per (sample, foreground channel), and a backward that routes the
gradient as torch autograd routes it through the reference's max-pools, minimums and relus.  CPU tensors run `soft_skeleton_torch`,
a restatement of the reference's functions, as the other non-fused loss terms do.  The activation, clamps, channel selection and
the final clDice formula on the (N, C) sums stay torch ops on the device.

Validation reads every min / max it needs (prediction, dense target or class-index labels) in one host synchronisation per call.
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .hip_dispatch import wants_hip


# ---- restatement of the reference's soft morphology (losses.py:47-85) -------------------------------------------------------------
def _soft_erode_pool(prob: torch.Tensor) -> torch.Tensor:
    if prob.ndim == 5:
        p1 = -F.max_pool3d(-prob, kernel_size=(3, 1, 1), stride=1, padding=(1, 0, 0))
        p2 = -F.max_pool3d(-prob, kernel_size=(1, 3, 1), stride=1, padding=(0, 1, 0))
        p3 = -F.max_pool3d(-prob, kernel_size=(1, 1, 3), stride=1, padding=(0, 0, 1))
        return torch.minimum(torch.minimum(p1, p2), p3)
    if prob.ndim == 4:
        p1 = -F.max_pool2d(-prob, kernel_size=(3, 1), stride=1, padding=(1, 0))
        p2 = -F.max_pool2d(-prob, kernel_size=(1, 3), stride=1, padding=(0, 1))
        return torch.minimum(p1, p2)
    raise ValueError(f"Expected 4D/5D tensor for soft erosion, got shape {tuple(prob.shape)}")


def _soft_dilate_pool(prob: torch.Tensor) -> torch.Tensor:
    if prob.ndim == 5:
        return F.max_pool3d(prob, kernel_size=3, stride=1, padding=1)
    if prob.ndim == 4:
        return F.max_pool2d(prob, kernel_size=3, stride=1, padding=1)
    raise ValueError(f"Expected 4D/5D tensor for soft dilation, got shape {tuple(prob.shape)}")


def soft_skeleton_torch(prob: torch.Tensor, num_iters: int) -> torch.Tensor:
    """`_soft_skeletonize_pool` of the reference, op for op (differentiable through torch autograd)."""
    opened = _soft_dilate_pool(_soft_erode_pool(prob))
    skeleton = F.relu(prob - opened)
    for _ in range(num_iters):
        prob = _soft_erode_pool(prob)
        opened = _soft_dilate_pool(_soft_erode_pool(prob))
        delta = F.relu(prob - opened)
        skeleton = skeleton + F.relu(delta - skeleton * delta)
    return skeleton


def _sums_torch(pred_fg, target_fg, fg_weight, num_iters: int):
    """(pred-skeleton sums, target-skeleton sums), each (N, C, 2), as the reference forms them."""
    pred_skeleton = soft_skeleton_torch(pred_fg, num_iters)
    target_skeleton = soft_skeleton_torch(target_fg, num_iters)
    if fg_weight is not None:
        pred_eval, target_eval = pred_fg * fg_weight, target_fg * fg_weight
        pred_skeleton_eval, target_skeleton_eval = pred_skeleton * fg_weight, target_skeleton * fg_weight
    else:
        pred_eval, target_eval = pred_fg, target_fg
        pred_skeleton_eval, target_skeleton_eval = pred_skeleton, target_skeleton
    dims = tuple(range(2, pred_fg.ndim))
    ps = torch.stack([(pred_skeleton_eval * target_eval).sum(dim=dims), pred_skeleton_eval.sum(dim=dims)], -1)
    ts = torch.stack([(target_skeleton_eval * pred_eval).sum(dim=dims), target_skeleton_eval.sum(dim=dims)], -1)
    return ps, ts


class _ClDiceSums(torch.autograd.Function):
    """prob, target, weight (N, C, ...) fp32 contiguous -> ps = (sum (S_p w)(t w), sum S_p w), ts = (sum (S_t w)(p w), sum S_t w),
    each (N, C, 2).  Differentiable in prob only."""

    @staticmethod
    def forward(ctx, prob, target, weight, num_iters: int):
        from .. import hip_ops as ops
        P = ops.cldice_levels(prob, num_iters)
        _, ps = ops.cldice_skeleton(prob, P, num_iters, other=target, weight=weight, want_skeleton=False)
        Pt = ops.cldice_levels(target, num_iters)
        skel_t, ts = ops.cldice_skeleton(target, Pt, num_iters, other=prob, weight=weight)
        del Pt
        ctx.num_iters = int(num_iters)
        ctx.save_for_backward(prob, P, target, weight, skel_t)
        return ps, ts

    @staticmethod
    def backward(ctx, g_ps, g_ts):
        from .. import hip_ops as ops
        prob, P, target, weight, skel_t = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        zero = prob.new_zeros(prob.shape[:2])
        alpha, beta = (g_ps[..., 0], g_ps[..., 1]) if g_ps is not None else (zero, zero)
        gamma = g_ts[..., 0] if g_ts is not None else zero
        coef = torch.stack([alpha, beta, gamma]).float().contiguous()
        grad = ops.cldice_backward(prob, P, ctx.num_iters, target, weight, coef, skel_t if g_ts is not None else None)
        return grad, None, None, None


class SoftClDiceLoss(nn.Module):
    """Soft clDice loss (the reference's SoftClDiceLoss: same arguments, defaults, checks and messages).  `use_hip`: None picks the
    HIP kernels for CUDA tensors and the torch restatement for CPU tensors; False forces the restatement (tests, probes); True on
    CPU tensors is an error."""

    def __init__(self, num_iters: int = 5, mode: str = "binary", reduction: str = "mean", smooth: float = 1.0,
                 foreground_channel: int = 1, background_index: int = 0, sigmoid: bool = False, softmax: bool = False,
                 clamp_probabilities: bool = False, validate_inputs: bool = True, validation_tolerance: float = 1e-5,
                 use_hip: Optional[bool] = None):
        super().__init__()
        if num_iters < 0:
            raise ValueError(f"num_iters must be >= 0, got {num_iters}")
        if mode not in {"binary", "multi"}:
            raise ValueError(f"mode must be 'binary' or 'multi', got {mode!r}")
        if reduction not in {"none", "mean", "sum"}:
            raise ValueError(f"reduction must be 'none', 'mean', or 'sum', got {reduction!r}")
        if smooth <= 0:
            raise ValueError(f"smooth must be > 0, got {smooth}")
        if sigmoid and softmax:
            raise ValueError("sigmoid and softmax are mutually exclusive")
        if validation_tolerance < 0:
            raise ValueError(f"validation_tolerance must be >= 0, got {validation_tolerance}")
        self.num_iters = int(num_iters)
        self.mode = mode
        self.reduction = reduction
        self.smooth = float(smooth)
        self.foreground_channel = int(foreground_channel)
        self.background_index = int(background_index)
        self.sigmoid = bool(sigmoid)
        self.softmax = bool(softmax)
        self.clamp_probabilities = bool(clamp_probabilities)
        self.validate_inputs = bool(validate_inputs)
        self.validation_tolerance = float(validation_tolerance)
        self.use_hip = use_hip

    # ---- the reference's helpers, with the host reads gathered into one synchronisation ------------------------------------------
    def _apply_activation(self, pred):
        if self.sigmoid:
            return torch.sigmoid(pred)
        if self.softmax:
            if pred.shape[1] < 2:
                raise ValueError("softmax=True requires prediction with at least 2 channels")
            return F.softmax(pred, dim=1)
        return pred

    @staticmethod
    def _check_target_shape(target, pred):
        """-> (target with a channel axis, True when it is a class-index target to one-hot encode)."""
        if target.ndim == pred.ndim - 1:
            target = target.unsqueeze(1)
        if target.ndim != pred.ndim:
            raise ValueError(f"Target ndim ({target.ndim}) does not match prediction ndim ({pred.ndim})")
        if target.shape[0] != pred.shape[0] or target.shape[2:] != pred.shape[2:]:
            raise ValueError("Target shape must match prediction shape except for channel dimension: "
                             f"target={tuple(target.shape)}, pred={tuple(pred.shape)}")
        if target.shape[1] == pred.shape[1]:
            return target, False
        if target.shape[1] == 1 and pred.shape[1] > 1:
            return target, True
        raise ValueError("Target channel count is incompatible with prediction: "
                         f"target_channels={target.shape[1]}, pred_channels={pred.shape[1]}")

    def _range_error(self, name, lo, hi):
        tol = self.validation_tolerance
        if lo < -tol or hi > (1.0 + tol):
            raise ValueError(f"{name} must be probabilities in [0, 1] (tolerance={tol}), got min={lo:.6f}, max={hi:.6f}. "
                             "Pass sigmoid=True/softmax=True for logits.")

    def _select_foreground_channels(self, pred, target):
        channels = pred.shape[1]
        if self.mode == "binary":
            fg_idx = 0 if channels == 1 else self.foreground_channel
            if fg_idx < 0 or fg_idx >= channels:
                raise ValueError(f"foreground_channel={self.foreground_channel} is invalid for {channels} channels")
            return pred[:, fg_idx:fg_idx + 1], target[:, fg_idx:fg_idx + 1], [fg_idx]
        if channels == 1:
            return pred, target, [0]
        background_index = self.background_index
        if background_index < 0:
            background_index += channels
        if background_index < 0 or background_index >= channels:
            raise ValueError(f"background_index={self.background_index} is invalid for {channels} channels")
        foreground_indices = [idx for idx in range(channels) if idx != background_index]
        if not foreground_indices:
            raise ValueError(f"No foreground classes available: channels={channels}, background_index={self.background_index}")
        index_tensor = torch.tensor(foreground_indices, device=pred.device, dtype=torch.long)
        return (torch.index_select(pred, dim=1, index=index_tensor), torch.index_select(target, dim=1, index=index_tensor),
                foreground_indices)

    @staticmethod
    def _prepare_weight(weight, pred, foreground_indices: List[int], num_fg_channels: int):
        if weight.ndim == pred.ndim - 1:
            weight = weight.unsqueeze(1)
        if weight.ndim != pred.ndim:
            raise ValueError(f"Weight ndim ({weight.ndim}) must match pred ndim ({pred.ndim})")
        if weight.shape[0] != pred.shape[0] or weight.shape[2:] != pred.shape[2:]:
            raise ValueError("Weight shape must match prediction shape except for channel dimension: "
                             f"weight={tuple(weight.shape)}, pred={tuple(pred.shape)}")
        weight = weight.to(device=pred.device, dtype=pred.dtype)
        if weight.shape[1] == num_fg_channels:
            return weight
        if weight.shape[1] == 1:
            return weight.expand(weight.shape[0], num_fg_channels, *weight.shape[2:])
        if weight.shape[1] == pred.shape[1]:
            if num_fg_channels == pred.shape[1]:
                return weight
            index_tensor = torch.tensor(foreground_indices, device=pred.device, dtype=torch.long)
            return torch.index_select(weight, dim=1, index=index_tensor)
        raise ValueError("Weight channel count must be 1, foreground-channel count, or prediction-channel count; "
                         f"got {weight.shape[1]}")

    def forward(self, pred: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        if pred.ndim not in {4, 5}:
            raise ValueError(f"SoftClDiceLoss expects 4D/5D tensors, got {tuple(pred.shape)}")
        hip = wants_hip(self.use_hip, pred, "SoftClDiceLoss")

        pred = self._apply_activation(pred)
        target, class_index = self._check_target_shape(target, pred)
        if self.clamp_probabilities:
            pred = pred.clamp(0.0, 1.0)
        labels = None
        if class_index:
            labels = target.squeeze(1).long()
        else:
            target = target.to(device=pred.device, dtype=pred.dtype)
            if self.clamp_probabilities:
                target = target.clamp(0.0, 1.0)
        # every min / max the checks below need, read in one host synchronisation
        stats = []
        if labels is not None:
            stats += [labels.min(), labels.max()]
        if self.validate_inputs:
            stats += [pred.detach().min(), pred.detach().max()]
            if labels is None:
                stats += [target.min(), target.max()]
        host = torch.stack([s.to(torch.float64) for s in stats]).tolist() if stats else []
        if labels is not None:
            min_label, max_label = int(host[0]), int(host[1])
            host = host[2:]
            if min_label < 0 or max_label >= pred.shape[1]:
                raise ValueError(f"Class-index targets must be in [0, {pred.shape[1] - 1}], got min={min_label}, max={max_label}")
            target = F.one_hot(labels, num_classes=pred.shape[1]).movedim(-1, 1).to(device=pred.device, dtype=pred.dtype)
            if self.clamp_probabilities:
                target = target.clamp(0.0, 1.0)
        if self.validate_inputs:
            spatial_shape = tuple(pred.shape[2:])
            if any(dim < 3 for dim in spatial_shape):
                raise ValueError("SoftClDiceLoss expects each spatial dimension >= 3 for stable morphology, "
                                 f"got spatial shape {spatial_shape}")
            self._range_error("pred", host[0], host[1])
            if labels is None:
                self._range_error("target", host[2], host[3])

        pred_fg, target_fg, foreground_indices = self._select_foreground_channels(pred, target)
        if self.clamp_probabilities:
            pred_fg = pred_fg.clamp(0.0, 1.0)
            target_fg = target_fg.clamp(0.0, 1.0)
        fg_weight = None
        if weight is not None:
            fg_weight = self._prepare_weight(weight, pred, foreground_indices, pred_fg.shape[1])
            if self.clamp_probabilities:
                fg_weight = fg_weight.clamp_min(0.0)

        if hip:
            w = fg_weight.detach().float().contiguous() if fg_weight is not None else None
            ps, ts = _ClDiceSums.apply(pred_fg.float().contiguous(), target_fg.detach().float().contiguous(), w, self.num_iters)
        else:
            ps, ts = _sums_torch(pred_fg, target_fg, fg_weight, self.num_iters)

        topology_precision = (ps[..., 0] + self.smooth) / (ps[..., 1] + self.smooth)
        topology_sensitivity = (ts[..., 0] + self.smooth) / (ts[..., 1] + self.smooth)
        cl_dice = 2.0 * topology_precision * topology_sensitivity / (topology_precision + topology_sensitivity + self.smooth)
        loss = 1.0 - cl_dice
        if self.reduction == "none":
            return loss
        if self.reduction == "sum":
            return loss.sum()
        return loss.mean()


"""The reference's regularisation losses (connectomics/models/losses/regularization.py) with value and gradients on HIP
(csrc/regularization_kernels.hip): BinaryRegularization, ForegroundDistanceConsistency, ContourDistanceConsistency,
ForegroundContourConsistency and NonOverlapRegularization -- same names, arguments, defaults, checks and messages, plus `use_hip`.

None of them takes a target: a `pred_only` loss sees one prediction slice, a `pred_pred` loss two (models/losses/metadata.py:53-76);
those with a `mask` argument multiply the per-voxel loss by it before the mean.

CUDA tensors run the kernels: one forward pass writes the sum of mask x loss from fixed-order partials, the value is sum / numel
formed on the device (numel = the element count of the broadcast loss x mask, what `.mean()` divides by), and one backward pass
recomputes everything from the inputs and writes every input's gradient -- nothing is saved but the inputs themselves and, for the
foreground / contour loss, a one-byte map of which window position supplied each pooled edge.  CPU tensors run the `*_torch`
restatements, which follow the reference op for op in the dtype they are given (the GPU tests run them in fp32 and fp64).

`use_hip`: None picks the kernels for CUDA tensors and the restatement for CPU tensors; False forces the restatement; True on CPU
tensors is an error.

Deviations from the reference: ForegroundContourConsistency takes 5-D single-channel inputs only (the reference's conv3d would read
a 4-D input as unbatched), and a mask that does not broadcast to the loss is refused (the reference would silently enlarge the
loss to the mask's shape).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .hip_dispatch import checked_mask, kernel_mask, wants_hip


# ---- the torch restatements (the CPU path, and the yardstick of the GPU tests) -----------------------------------------------------
def binary_regularization_torch(pred, mask=None, *, min_threshold: float = 1e-2, apply_sigmoid: bool = True):
    prob = torch.sigmoid(pred) if apply_sigmoid else pred
    loss = 1.0 / torch.clamp(torch.abs(prob - 0.5), min=min_threshold)
    if mask is not None:
        loss = loss * mask
    return loss.mean()


def foreground_distance_consistency_torch(foreground_logits, distance_transform, mask=None):
    log_pos, log_neg = F.logsigmoid(foreground_logits), F.logsigmoid(-foreground_logits)
    dist = torch.tanh(distance_transform)
    inside, outside = torch.clamp(dist, min=0.0), -torch.clamp(dist, max=0.0)
    loss = -log_pos * inside + -log_neg * outside
    if mask is not None:
        loss = loss * mask
    return loss.mean()


def contour_distance_consistency_torch(contour_logits, distance_transform, mask=None):
    contour_prob = torch.sigmoid(contour_logits)
    distance_abs = torch.abs(torch.tanh(distance_transform))
    if contour_prob.shape != distance_abs.shape:
        raise ValueError(f"Shape mismatch: contour_prob={contour_prob.shape} vs distance_abs={distance_abs.shape}")
    loss = (contour_prob * distance_abs) ** 2
    if mask is not None:
        loss = loss * mask
    return loss.mean()


def foreground_contour_edge_torch(foreground_logits, *, kernel_size: int = 3, eps: float = 1e-7):
    """The pooled edge map E of ForegroundContourConsistency: the clamped [1, 0, -1] gradient magnitude of sigmoid(fg) per z-plane,
    zero-padded by one voxel in y and x and max-pooled over kernel_size^2 (stride 1)."""
    prob = torch.sigmoid(foreground_logits)
    tap = torch.tensor([1.0, 0.0, -1.0], dtype=prob.dtype, device=prob.device)
    ex = F.conv3d(prob, tap.view(1, 1, 1, 1, 3), padding=(0, 0, 1))
    ey = F.conv3d(prob, tap.view(1, 1, 1, 3, 1), padding=(0, 1, 0))
    edge = torch.clamp(torch.sqrt(ex ** 2 + ey ** 2 + eps), min=eps, max=1.0 - eps)
    edge = F.pad(edge, (1, 1, 1, 1, 0, 0))
    return F.max_pool3d(edge, kernel_size=(1, kernel_size, kernel_size), stride=1)


def foreground_contour_consistency_torch(foreground_logits, contour_logits, mask=None, *, kernel_size: int = 3, eps: float = 1e-7):
    contour_prob = torch.sigmoid(contour_logits)
    edge = foreground_contour_edge_torch(foreground_logits, kernel_size=kernel_size, eps=eps)
    if edge.shape != contour_prob.shape:
        raise ValueError(f"Shape mismatch: edge={edge.shape} vs contour_prob={contour_prob.shape}")
    loss = F.mse_loss(edge, contour_prob, reduction="none")
    if mask is not None:
        loss = loss * mask
    return loss.mean()


def non_overlap_regularization_torch(pred, *, cleft_masked: bool = True):
    if pred.shape[1] < 2:
        raise ValueError(f"Expected at least 2 channels for pre/post predictions, got {pred.shape[1]}")
    loss = torch.sigmoid(pred[:, 0]) * torch.sigmoid(pred[:, 1])
    if cleft_masked and pred.shape[1] >= 3:
        loss = loss * torch.sigmoid(pred[:, 2].detach())
    return loss.mean()


# ---- autograd over the kernels: one Function per loss ------------------------------------------------------------------------------
def _pointwise_function(kind: str, name: str):
    """The autograd Function of one streaming kind: (a, b or None, mask or None, param, flag, numel) -> sum / numel."""

    class _Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, a, b, mask, param: float, flag: bool, numel: int):
            from .. import hip_ops as ops
            total = ops.reg_pointwise_forward(kind, a, b, mask, param=param, flag=flag)
            ctx.save_for_backward(a, b, mask)
            ctx.param, ctx.flag, ctx.numel = float(param), bool(flag), int(numel)
            return (total / float(numel)).reshape(())

        @staticmethod
        def backward(ctx, g):
            from .. import hip_ops as ops
            a, b, mask = ctx.saved_tensors
            coef = (g.float() / float(ctx.numel)).reshape(1)
            da, db = ops.reg_pointwise_backward(kind, coef, a, b, mask, param=ctx.param, flag=ctx.flag)
            return da, db, None, None, None, None

    _Fn.__name__ = _Fn.__qualname__ = name
    return _Fn


_BinaryRegularizationFn = _pointwise_function("binary", "_BinaryRegularizationFn")
_ForegroundDistanceFn = _pointwise_function("fg_dist", "_ForegroundDistanceFn")
_ContourDistanceFn = _pointwise_function("ct_dist", "_ContourDistanceFn")
_NonOverlapFn = _pointwise_function("nonoverlap", "_NonOverlapFn")


class _ForegroundContourFn(torch.autograd.Function):
    """(fg, contour, mask or None, eps) -> mean of (E - sigmoid(contour))^2 mask; saves the inputs and the uint8 code map."""

    @staticmethod
    def forward(ctx, fg, contour, mask, eps: float):
        from .. import hip_ops as ops
        total, code = ops.fgcontour_forward(fg, contour, mask, eps=eps)
        ctx.save_for_backward(fg, contour, mask, code)
        ctx.eps = float(eps)
        return (total / float(fg.numel())).reshape(())

    @staticmethod
    def backward(ctx, g):
        from .. import hip_ops as ops
        fg, contour, mask, code = ctx.saved_tensors
        coef = (g.float() / float(fg.numel())).reshape(1)
        dfg, dct = ops.fgcontour_backward(coef, fg, contour, mask, code, eps=ctx.eps)
        return dfg, dct, None, None


def _operand(x: torch.Tensor) -> torch.Tensor:
    return x.float().contiguous()


def _two_operands(name: str, a: torch.Tensor, b: torch.Tensor):
    if a.shape != b.shape:                     # the reference broadcasts here; the kernels read two operands of one shape
        a, b = torch.broadcast_tensors(a, b)
    if a.dim() < 2:
        raise ValueError(f"{name} expects (N, C, ...) predictions, got {tuple(a.shape)}")
    return _operand(a), _operand(b)


# ---- the loss classes ----------------------------------------------------------------------------------------------------------------
class BinaryRegularization(nn.Module):
    """1 / max(|sigmoid(pred) - 0.5|, min_threshold), times the mask, averaged: pushes predictions away from 0.5."""

    def __init__(self, min_threshold: float = 1e-2, apply_sigmoid: bool = True, use_hip: Optional[bool] = None):
        super().__init__()
        self.min_threshold = min_threshold
        self.apply_sigmoid = apply_sigmoid
        self.use_hip = use_hip

    def forward(self, pred: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        mask = checked_mask(mask, pred.shape, "BinaryRegularization")
        if not wants_hip(self.use_hip, pred, "BinaryRegularization"):
            return binary_regularization_torch(pred, mask, min_threshold=self.min_threshold, apply_sigmoid=self.apply_sigmoid)
        if pred.dim() < 2:
            raise ValueError(f"BinaryRegularization expects (N, C, ...) predictions, got {tuple(pred.shape)}")
        x = _operand(pred)
        return _BinaryRegularizationFn.apply(x, None, kernel_mask(mask, x), float(self.min_threshold), bool(self.apply_sigmoid), x.numel())


class ForegroundDistanceConsistency(nn.Module):
    """-logsigmoid(fg) max(tanh d, 0) - logsigmoid(-fg) max(-tanh d, 0): foreground where the signed distance is positive."""

    def __init__(self, use_hip: Optional[bool] = None):
        super().__init__()
        self.use_hip = use_hip

    def forward(self, foreground_logits: torch.Tensor, distance_transform: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        shape = torch.broadcast_shapes(tuple(foreground_logits.shape), tuple(distance_transform.shape))
        mask = checked_mask(mask, shape, "ForegroundDistanceConsistency")
        if not wants_hip(self.use_hip, foreground_logits, "ForegroundDistanceConsistency"):
            return foreground_distance_consistency_torch(foreground_logits, distance_transform, mask)
        a, b = _two_operands("ForegroundDistanceConsistency", foreground_logits, distance_transform)
        return _ForegroundDistanceFn.apply(a, b, kernel_mask(mask, a), 0.0, True, a.numel())


class ContourDistanceConsistency(nn.Module):
    """(sigmoid(contour) |tanh d|)^2: contours where the distance transform is near zero."""

    def __init__(self, use_hip: Optional[bool] = None):
        super().__init__()
        self.use_hip = use_hip

    def forward(self, contour_logits: torch.Tensor, distance_transform: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        if contour_logits.shape != distance_transform.shape:
            raise ValueError(f"Shape mismatch: contour_prob={contour_logits.shape} vs distance_abs={distance_transform.shape}")
        mask = checked_mask(mask, contour_logits.shape, "ContourDistanceConsistency")
        if not wants_hip(self.use_hip, contour_logits, "ContourDistanceConsistency"):
            return contour_distance_consistency_torch(contour_logits, distance_transform, mask)
        a, b = _two_operands("ContourDistanceConsistency", contour_logits, distance_transform)
        return _ContourDistanceFn.apply(a, b, kernel_mask(mask, a), 0.0, True, a.numel())


class ForegroundContourConsistency(nn.Module):
    """(E - sigmoid(contour))^2 with E the 3 x 3 in-plane maximum of the clamped [1, 0, -1] gradient magnitude of sigmoid(fg).
    As in the reference only kernel_half_size = 1 keeps the pooled map the size of the contour map; another value raises the
    reference's shape-mismatch error from forward."""

    def __init__(self, kernel_half_size: int = 1, eps: float = 1e-7, use_hip: Optional[bool] = None):
        super().__init__()
        self.kernel_size = 2 * kernel_half_size + 1
        self.eps = eps
        self.use_hip = use_hip
        tap = torch.tensor([1.0, 0.0, -1.0])
        self.register_buffer("sobel_x", tap.view(1, 1, 1, 1, 3))
        self.register_buffer("sobel_y", tap.view(1, 1, 1, 3, 1))

    def forward(self, foreground_logits: torch.Tensor, contour_logits: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        if foreground_logits.dim() != 5 or foreground_logits.shape[1] != 1:
            raise ValueError("ForegroundContourConsistency takes 5-D single-channel foreground logits (N, 1, D, H, W), got "
                             f"{tuple(foreground_logits.shape)}")
        hip = wants_hip(self.use_hip, foreground_logits, "ForegroundContourConsistency")
        if self.kernel_size != 3 or contour_logits.shape != foreground_logits.shape or not hip:
            # (any kernel size but 3, or a contour map of another shape, ends in the reference's shape-mismatch error)
            if self.kernel_size == 3 and contour_logits.shape == foreground_logits.shape:
                mask = checked_mask(mask, foreground_logits.shape, "ForegroundContourConsistency")
            return foreground_contour_consistency_torch(foreground_logits, contour_logits, mask, kernel_size=self.kernel_size, eps=self.eps)
        mask = checked_mask(mask, foreground_logits.shape, "ForegroundContourConsistency")
        fg = _operand(foreground_logits)
        return _ForegroundContourFn.apply(fg, _operand(contour_logits), kernel_mask(mask, fg), float(self.eps))


class NonOverlapRegularization(nn.Module):
    """sigmoid(pre) sigmoid(post), times sigmoid(cleft) (detached) when cleft_masked and a third channel exists: channels 0, 1, 2."""

    def __init__(self, cleft_masked: bool = True, use_hip: Optional[bool] = None):
        super().__init__()
        self.cleft_masked = cleft_masked
        self.use_hip = use_hip

    def forward(self, pred: torch.Tensor) -> torch.Tensor:
        if pred.dim() < 2 or pred.shape[1] < 2:
            raise ValueError(f"Expected at least 2 channels for pre/post predictions, got {pred.shape[1] if pred.dim() >= 2 else 0}")
        if not wants_hip(self.use_hip, pred, "NonOverlapRegularization"):
            return non_overlap_regularization_torch(pred, cleft_masked=self.cleft_masked)
        x = _operand(pred)
        return _NonOverlapFn.apply(x, None, None, 0.0, bool(self.cleft_masked), x.numel() // x.shape[1])


__all__ = ["BinaryRegularization", "ForegroundDistanceConsistency", "ContourDistanceConsistency", "ForegroundContourConsistency",
           "NonOverlapRegularization"]

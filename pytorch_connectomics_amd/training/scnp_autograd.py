"""ScnpLoss: the reference's Same-Class Neighbor Penalization loss (connectomics/models/losses/losses.py:354-453) with the
neighbour-penalised logits, the BCE sums and the gradient on HIP (csrc/scnp_kernels.hip).

Every voxel's logit is replaced by its worst same-class neighbour of an ns^3 (2-D: ns^2) window -- the minimum over the foreground
neighbours for a foreground centre (target > 0.5), the maximum over the background neighbours otherwise -- and the result is scored
by the per-channel class-balanced BCE of `PerChannelBCEWithLogitsLoss`.

CUDA tensors run the kernels: one forward pass writes the supplier map and five sums per (sample, channel), a handful of torch ops on
(N, C) tensors turn them into the loss without a host synchronisation, and the backward gathers the gradient in a fixed order (no
atomics: bit-reproducible).  CPU tensors run `scnp_logits_torch`, a restatement of the reference's two gated max-pools, followed by
`per_channel_bce_with_logits`, as the other non-fused loss terms do.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .hip_dispatch import kernel_mask, wants_hip
from .losses import per_channel_bce_with_logits

_LARGE = 9999.0


def scnp_logits_torch(logits: torch.Tensor, target: torch.Tensor, neighborhood_size: int) -> torch.Tensor:
    """`ScnpLoss._scnp_logits` of the reference (losses.py:414-437), op for op (differentiable through torch autograd)."""
    ns = int(neighborhood_size)
    if logits.ndim == 5:
        mp = F.max_pool3d
        kernel = (ns, ns, ns)
        pad = (ns // 2, ns // 2, ns // 2)
    elif logits.ndim == 4:
        mp = F.max_pool2d
        kernel = (ns, ns)
        pad = (ns // 2, ns // 2)
    else:
        raise ValueError(f"ScnpLoss expects 4D [B,C,H,W] or 5D [B,C,Z,Y,X] logits, got {logits.ndim}D.")
    fg = (target > 0.5).to(logits.dtype)
    bg = 1.0 - fg
    t1 = -mp(-(logits * fg + _LARGE * bg), kernel, 1, pad)
    t2 = mp(logits * bg - _LARGE * fg, kernel, 1, pad)
    return t1 * fg + t2 * bg


class _ScnpSums(torch.autograd.Function):
    """logits, target (N, C, ...) and weight ((N, C, ...), (N, 1, ...) or None), fp32 contiguous ->
    (bce (N, C) = sum over the volume of w bce_pw(z~, t), valid (N, C) int32 = the count of w > 0), pw the per-channel
    min(n_neg / n_pos, max_pos_weight) of the batch (1 without positives, or with auto_pos_weight off).  Differentiable in the
    logits only."""

    @staticmethod
    def forward(ctx, logits, target, weight, ns: int, auto_pos_weight: bool, max_pos_weight: float, valid_only: bool):
        from .. import hip_ops as ops
        arg, sums, counts, _ = ops.scnp_forward(logits, target, weight, ns, valid_only=valid_only)
        C = logits.shape[1]
        if auto_pos_weight:
            pos = counts[..., 1].sum(0).float()
            neg = counts[..., 2].sum(0).float()
            ratio = torch.clamp(neg / pos.clamp_min(1.0), max=float(max_pos_weight))
            pw = torch.where(pos > 0, ratio, torch.ones_like(ratio))
        else:
            pw = torch.ones(C, dtype=torch.float32, device=logits.device)
        ctx.ns, ctx.valid_only = int(ns), bool(valid_only)
        ctx.save_for_backward(logits, target, weight, arg, pw)
        valid = counts[..., 0].contiguous()
        ctx.mark_non_differentiable(valid)
        return sums[..., 0] + (pw - 1.0) * sums[..., 1], valid

    @staticmethod
    def backward(ctx, g_bce, _g_valid):
        from .. import hip_ops as ops
        logits, target, weight, arg, pw = ctx.saved_tensors
        if not ctx.needs_input_grad[0] or g_bce is None:
            return (None,) * 7
        N, C = logits.shape[:2]
        grad = ops.scnp_backward(logits, target, weight, arg, g_bce.float().contiguous(), pw.expand(N, C).contiguous(), ctx.ns,
                                 valid_only=ctx.valid_only)
        return (grad,) + (None,) * 6


class ScnpLoss(nn.Module):
    """Same-Class Neighbor Penalization loss (the reference's ScnpLoss: same arguments, defaults, checks and messages).  `use_hip`:
    None picks the HIP kernels for CUDA tensors and the torch restatement for CPU tensors; False forces the restatement (tests,
    probes); True on CPU tensors is an error.  The kernels are built for neighborhood_size 1, 3, 5 and 7; the restatement takes any
    odd size.  `reduction` is 'mean' or 'sum' per channel (the channels are summed).  The kernels read a weight of shape (N, C, ...)
    or (N, 1, ...) as it is; a weight of any other shape that broadcasts to the logits' (the restatement multiplies by it) is expanded
    to (N, C, ...) first, and one that does not broadcast fails in that expansion."""

    def __init__(self, neighborhood_size: int = 3, auto_pos_weight: bool = True, max_pos_weight: float = 10.0,
                 reduction: str = "mean", use_hip: Optional[bool] = None):
        super().__init__()
        if neighborhood_size < 1 or neighborhood_size % 2 == 0:
            raise ValueError(f"neighborhood_size must be a positive odd int, got {neighborhood_size}.")
        if reduction not in ("mean", "sum"):
            raise ValueError(f"ScnpLoss reduction must be 'mean' or 'sum', got {reduction!r}: a training loss term must reduce to "
                             "one value")
        self.neighborhood_size = int(neighborhood_size)
        self.auto_pos_weight = bool(auto_pos_weight)
        self.max_pos_weight = float(max_pos_weight)
        self.reduction = reduction
        self.use_hip = use_hip

    def forward(self, input: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        if input.ndim not in (4, 5):
            raise ValueError(f"ScnpLoss expects 4D [B,C,H,W] or 5D [B,C,Z,Y,X] logits, got {input.ndim}D.")
        x, t = input.float(), target.float()
        if not wants_hip(self.use_hip, input, "ScnpLoss"):
            return per_channel_bce_with_logits(scnp_logits_torch(x, t, self.neighborhood_size), t, weight,
                                               auto_pos_weight=self.auto_pos_weight, max_pos_weight=self.max_pos_weight,
                                               reduction=self.reduction)
        w = kernel_mask(weight, x)                     # (another broadcastable shape, e.g. (1, C, 1, 1, 1), is expanded)
        mean = self.reduction == "mean"
        # 'mean' averages weight * bce over the voxels of weight > 0; 'sum' adds every voxel's weight * bce, whatever its sign
        bce, valid = _ScnpSums.apply(x.contiguous(), t.detach().contiguous(), w, self.neighborhood_size, self.auto_pos_weight,
                                     self.max_pos_weight, mean)
        per_channel = bce.sum(0)
        if mean:
            per_channel = per_channel / valid.sum(0).clamp_min(1).float()
        return per_channel.sum()


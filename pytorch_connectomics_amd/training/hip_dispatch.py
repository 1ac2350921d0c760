"""What every loss with HIP kernels decides before it launches them: whether the kernels run at all, whether a mask fits the loss, and
the form in which the kernels read a mask or weight."""
from __future__ import annotations

from typing import Optional

import torch


def wants_hip(use_hip: Optional[bool], x: torch.Tensor, name: str) -> bool:
    """`use_hip` None: the kernels for CUDA tensors, the torch restatement for CPU tensors; False forces the restatement; True on CPU
    tensors is an error."""
    hip = x.is_cuda if use_hip is None else bool(use_hip)
    if hip and not x.is_cuda:
        raise RuntimeError(f"{name}(use_hip=True) needs CUDA(HIP) tensors: the HIP kernels have no CPU path")
    return hip


def checked_mask(mask: Optional[torch.Tensor], loss_shape, name: str) -> Optional[torch.Tensor]:
    """The mask as given, after the check that it broadcasts TO the loss (never enlarges it)."""
    if mask is None:
        return None
    try:
        ok = tuple(torch.broadcast_shapes(tuple(loss_shape), tuple(mask.shape))) == tuple(loss_shape)
    except RuntimeError:
        ok = False
    if not ok:
        raise ValueError(f"{name}: mask of shape {tuple(mask.shape)} does not broadcast to the loss of shape {tuple(loss_shape)}")
    return mask


def channel_mask(mask: Optional[torch.Tensor], like: torch.Tensor) -> Optional[torch.Tensor]:
    """A mask or weight in the shape the kernels read: the operand's batch and spatial dims with the operand's channels or one; any
    other shape that broadcasts to the operand's is expanded first (one that does not fails in that expansion)."""
    if mask is None:
        return None
    if mask.dim() != like.dim() or mask.shape[1] not in (1, like.shape[1]) or mask.shape[0] != like.shape[0] \
            or mask.shape[2:] != like.shape[2:]:
        mask = mask.expand_as(like)
    return mask


def kernel_mask(mask: Optional[torch.Tensor], like: torch.Tensor) -> Optional[torch.Tensor]:
    """The mask as the kernels read it: `channel_mask`, detached, fp32 and contiguous."""
    return None if mask is None else channel_mask(mask.detach().float(), like).contiguous()

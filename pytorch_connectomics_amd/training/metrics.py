"""The `evaluation` block's voxel metrics -- jaccard, dice, accuracy, binary and multi-class -- as functions of one K x K table of
integer counts (reference training/lightning/model.py:434-476, 912-1005; evaluation/metric_execution.py:166-220).

`ConfusionState` holds the table of one epoch: counts[t * K + p] = the voxels with target class t and predicted class p, K =
max(num_classes, 2), plus one cell of voxels whose class-index label lies outside [0, K).  CUDA tensors are counted by one call of the
HIP kernel pair (hip_ops.confusion_counts, csrc/metric_kernels.hip: no torch element-wise launch, no host synchronisation); CPU tensors
by `confusion_counts_torch`, the same counts from torch for any number of classes.  The counts are int64 and add exactly across
batches and, with `all_reduce`, across ranks; `compute` reads them once and forms the metrics in float64 on the host.

The formulas are the published definitions of the torchmetrics classes the reference constructs (model.py:443-476):
  binary (num_classes == 1): TP = c[1][1], FP = c[0][1], FN = c[1][0], TN = c[0][0];
      jaccard = TP / (TP + FP + FN), dice = 2 TP / (2 TP + FP + FN), accuracy = (TP + TN) / total, each 0 when its denominator is 0;
  multi-class: TP_k = c[k][k], FP_k = column sum - TP_k, FN_k = row sum - TP_k; jaccard and dice are the mean of the binary formulas
      over the classes with TP_k + FP_k + FN_k > 0 (macro; 0 when no class is present), accuracy = sum_k TP_k / total (micro).
Instance-level names (adapted_rand, voi, instance_accuracy, instance_accuracy_detail) need a decoded segmentation: test mode computes
them after its decoding step from a label-pair table on the device (`pytorch_connectomics_amd/metrics/`); any
name outside {jaccard, dice, accuracy} is ignored here, as the reference ignores it in validation.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional

import torch

VOXEL_METRICS = ("jaccard", "dice", "accuracy")
TARGET_MODES = ("index", "threshold", "dense")


def confusion_counts_torch(pred: torch.Tensor, target: torch.Tensor, *, target_mode: str = "index", pred_threshold: float = 0.5,
                           target_threshold: float = 0.5) -> torch.Tensor:
    """The table of `ConfusionState` from torch ops, for any C: K * K + 1 int64 on the operands' device.  pred (N, C, *spatial);
    target (N, *spatial) / (N, 1, *spatial) for "index" (a float truncated toward zero, as `.long()`) and "threshold" (C == 1:
    target > target_threshold), pred's shape for "dense" (argmax over the channels).  Predicted class: C == 1: pred > pred_threshold;
    else torch.argmax over the channels."""
    if target_mode not in TARGET_MODES:
        raise ValueError(f"target_mode must be one of {list(TARGET_MODES)}, got {target_mode!r}")
    if pred.dim() < 3:
        raise ValueError(f"the prediction must have shape (N, C, *spatial), got {tuple(pred.shape)}")
    C = int(pred.shape[1])
    K = max(C, 2)
    p = (pred[:, 0] > pred_threshold).long() if C == 1 else torch.argmax(pred, dim=1)
    if target_mode == "dense":
        if C < 2 or target.shape != pred.shape:
            raise ValueError(f"a dense target needs C >= 2 and the prediction's shape {tuple(pred.shape)}, got {tuple(target.shape)}")
        t = torch.argmax(target, dim=1)
        valid = torch.ones_like(t, dtype=torch.bool)
    else:
        if target.shape == pred.shape[:1] + (1,) + pred.shape[2:]:
            target = target[:, 0]
        if target.shape != p.shape:
            raise ValueError(f"target of shape {tuple(target.shape)} does not hold one class per voxel of the prediction {tuple(pred.shape)}")
        if target_mode == "threshold":
            if C != 1:
                raise ValueError(f"a threshold target needs a one-channel prediction, got C = {C}")
            t = (target > target_threshold).long()
            valid = torch.ones_like(t, dtype=torch.bool)
        else:
            if not target.dtype.is_floating_point:
                target = target.long()
            valid = (target > -1) & (target < K)                      # false for NaN; (-1, 0) truncates to class 0
            t = torch.where(valid, target, torch.zeros_like(target)).long()
    cells = torch.bincount((t * K + p)[valid].reshape(-1), minlength=K * K)
    return torch.cat([cells, (~valid).sum().reshape(1)]).to(torch.int64)


def metrics_from_counts(counts, num_classes: int, names: Iterable[str]) -> Dict[str, float]:
    """jaccard / dice / accuracy (those of `names`; other names are ignored) from a host table of K * K + 1 counts, in float64.
    ValueError when the table holds voxels whose label was outside [0, K)."""
    K = max(int(num_classes), 2)
    flat = [int(v) for v in (counts.tolist() if hasattr(counts, "tolist") else counts)]
    if len(flat) != K * K + 1:
        raise ValueError(f"a table for {num_classes} classes holds {K * K + 1} counts, got {len(flat)}")
    if flat[K * K] > 0:
        raise ValueError(f"{flat[K * K]} voxels carry a class label outside [0, {K}): the metrics are undefined on them")
    c = [flat[t * K:(t + 1) * K] for t in range(K)]
    total = float(sum(flat[:K * K]))

    def ratio(num: float, den: float) -> float:
        return float(num) / float(den) if den > 0 else 0.0

    tp = [float(c[k][k]) for k in range(K)]
    fp = [float(sum(c[t][k] for t in range(K))) - tp[k] for k in range(K)]
    fn = [float(sum(c[k])) - tp[k] for k in range(K)]
    out: Dict[str, float] = {}
    names = [n for n in names if n in VOXEL_METRICS]
    if int(num_classes) == 1:
        if "jaccard" in names:
            out["jaccard"] = ratio(tp[1], tp[1] + fp[1] + fn[1])
        if "dice" in names:
            out["dice"] = ratio(2 * tp[1], 2 * tp[1] + fp[1] + fn[1])
        if "accuracy" in names:
            out["accuracy"] = ratio(tp[1] + float(c[0][0]), total)
        return out
    present = [k for k in range(K) if tp[k] + fp[k] + fn[k] > 0]
    if "jaccard" in names:
        out["jaccard"] = ratio(sum(ratio(tp[k], tp[k] + fp[k] + fn[k]) for k in present), len(present))
    if "dice" in names:
        out["dice"] = ratio(sum(ratio(2 * tp[k], 2 * tp[k] + fp[k] + fn[k]) for k in present), len(present))
    if "accuracy" in names:
        out["accuracy"] = ratio(sum(tp), total)
    return out


def _kernel_target(target: torch.Tensor) -> torch.Tensor:
    """The label in a dtype the kernel reads (fp32, int64, uint8): one cast for any other."""
    if target.dtype in (torch.float32, torch.int64, torch.uint8):
        return target
    if target.dtype == torch.bool:
        return target.to(torch.uint8)
    return target.to(torch.float32 if target.dtype.is_floating_point else torch.int64)


class ConfusionState:
    """One epoch's table of counts for `num_classes` output channels (1 = a binary metric on a thresholded channel)."""

    def __init__(self, num_classes: int):
        if int(num_classes) < 1:
            raise ValueError(f"num_classes must be >= 1, got {num_classes}")
        self.num_classes = int(num_classes)
        self.K = max(self.num_classes, 2)
        self.counts: Optional[torch.Tensor] = None            # K * K + 1 int64, on the device of the first update

    def _table(self, device) -> torch.Tensor:
        if self.counts is None:
            self.counts = torch.zeros((self.K * self.K + 1,), dtype=torch.int64, device=device)
        elif self.counts.device != device:
            self.counts = self.counts.to(device)
        return self.counts

    def update(self, pred: torch.Tensor, target: torch.Tensor, *, pred_threshold: float = 0.5, target_mode: str = "index",
               target_threshold: float = 0.5) -> None:
        """Add one batch: pred (N, num_classes, *spatial) raw outputs, target as `confusion_counts_torch` describes.  CUDA: exactly one
        hip_ops.confusion_counts call on the tensors as they are (slices and channels-last views go by their strides)."""
        if pred.dim() < 3 or int(pred.shape[1]) != self.num_classes:
            raise ValueError(f"the prediction must have shape (N, {self.num_classes}, *spatial), got {tuple(pred.shape)}")
        counts = self._table(pred.device)
        pred, target = pred.detach(), target.detach()
        if pred.is_cuda:
            from .. import hip_ops as ops
            ops.confusion_counts(pred if pred.dtype == torch.float32 else pred.float(), _kernel_target(target), counts,
                                 target_mode=target_mode, pred_threshold=pred_threshold, target_threshold=target_threshold)
        else:
            counts += confusion_counts_torch(pred, target, target_mode=target_mode, pred_threshold=pred_threshold,
                                             target_threshold=target_threshold)

    def reset(self) -> None:
        if self.counts is not None:
            self.counts.zero_()

    def all_reduce(self) -> None:
        """SUM the table over the ranks when torch.distributed is initialised (integer adds: exact)."""
        if self.counts is not None and torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(self.counts, op=torch.distributed.ReduceOp.SUM)

    def table(self) -> torch.Tensor:
        """The counts on the host (one read)."""
        return torch.zeros((self.K * self.K + 1,), dtype=torch.int64) if self.counts is None else self.counts.cpu()

    def compute(self, names: Iterable[str]) -> Dict[str, float]:
        return metrics_from_counts(self.table(), self.num_classes, names)


__all__ = ["ConfusionState", "confusion_counts_torch", "metrics_from_counts", "VOXEL_METRICS", "TARGET_MODES"]

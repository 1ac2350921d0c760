"""adapted_rand, voi, instance_matching and instance_matching_simple with the reference's names and signatures
(metrics/segmentation_numpy.py), on the label-pair table of hip_ops.label_pair_table.  A device tensor is used where it lies; a numpy
array is uploaded.  What leaves the device is the table's 16-cell record and, for the matching, the pairs that pass the threshold.

Not built, refused by name: criteria `iot` / `iop`, `report_matches=True` and with it mean_matched_score, mean_true_score and
panoptic_quality (they need the optimal assignment itself, which the reference's evaluation does not report)."""
from __future__ import annotations

from typing import Iterable, Optional

import numpy as np

from .finalize import adapted_rand_from_record, matching_from_record, voi_from_record

INSTANCE_METRIC_NAMES = ("adapted_rand", "voi", "instance_accuracy", "instance_accuracy_detail")
_REFERENCE_CRITERIA = ("iou", "iot", "iop")


def _ids(x, name: str):
    import torch
    if isinstance(x, torch.Tensor):
        if not x.is_cuda:
            if not torch.cuda.is_available():
                raise RuntimeError(f"{name}: the instance metrics need an MI355X (ROCm) device: this engine has no CPU path")
            x = x.cuda()
        return x
    arr = np.asarray(x)
    if not np.issubdtype(arr.dtype, np.integer) and arr.dtype != np.bool_:
        raise ValueError(f"{name} must be an array of non-negative integers.")
    if arr.dtype not in (np.int32, np.int64):
        arr = arr.astype(np.int32 if arr.dtype.itemsize < 4 else np.int64)
    if not torch.cuda.is_available():
        raise RuntimeError(f"{name}: the instance metrics need an MI355X (ROCm) device: this engine has no CPU path")
    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


def _table(seg, gt):
    from .. import hip_ops
    return hip_ops.label_pair_table(_ids(seg, "seg"), _ids(gt, "gt"))


def _same_shape(seg, gt):
    if tuple(seg.shape) != tuple(gt.shape):
        raise ValueError(f"seg and gt must have the same shape. Got seg.shape={tuple(seg.shape)}, gt.shape={tuple(gt.shape)}")


def adapted_rand(seg, gt, all_stats: bool = False):
    """Adapted Rand error of the SNEMI3D contest, 1 - the F-score of the Rand index without the zero component of gt; with all_stats
    the tuple (are, precision, recall).  The reference's float64 values bit for bit."""
    _same_shape(seg, gt)
    return adapted_rand_from_record(_table(seg, gt).record(), all_stats)


def voi(reconstruction, groundtruth, ignore_reconstruction=None, ignore_groundtruth=None):
    """(split, merge) = (H(reconstruction | groundtruth), H(groundtruth | reconstruction)) over the voxels whose ground truth is not 0;
    id 0 of the reconstruction is an ordinary label.  Other ignore lists than the reference's defaults are not built."""
    if ignore_reconstruction not in (None, [], ()) or ignore_groundtruth not in (None, [0], (0,)):
        raise NotImplementedError(f"voi with ignore_reconstruction={ignore_reconstruction}, ignore_groundtruth={ignore_groundtruth} is not "
                                  "built: only the defaults ([] and [0]) are")
    _same_shape(reconstruction, groundtruth)
    return voi_from_record(_table(reconstruction, groundtruth).record())


def _check_matching(y_true, y_pred, criterion, report_matches=False):
    if tuple(y_true.shape) != tuple(y_pred.shape):
        raise ValueError(f"y_true ({tuple(y_true.shape)}) and y_pred ({tuple(y_pred.shape)}) have different shapes")
    if criterion not in _REFERENCE_CRITERIA:
        raise ValueError("Matching criterion '%s' not supported." % criterion)
    if criterion != "iou":
        raise NotImplementedError(f"Matching criterion '{criterion}' is not built: only 'iou' is")
    if report_matches:
        raise NotImplementedError("report_matches=True (the optimal assignment itself, matched pairs and scores) is not built")


def instance_matching(y_true, y_pred, thresh: float = 0.5, criterion: str = "iou", report_matches: bool = False):
    """Detection metrics of the optimal matching between ground-truth and predicted objects: tp is the largest number of disjoint
    (gt, pred) pairs with IoU >= thresh.  Keys: criterion, thresh, fp, tp, fn, precision, recall, accuracy, f1, n_true, n_pred."""
    _check_matching(y_true, y_pred, criterion, report_matches)
    thresh = 0.0 if thresh is None else float(thresh)
    table = _table(y_pred, y_true)
    pairs, _ = table.matches(thresh)
    return matching_from_record(table.record(), pairs, thresh, criterion)


def instance_matching_simple(y_true, y_pred, thresh: float = 0.5, criterion: str = "iou"):
    """The relaxed count: every (gt, pred) pair with IoU >= thresh is a true positive, no matching."""
    _check_matching(y_true, y_pred, criterion)
    thresh = float(thresh)
    table = _table(y_pred, y_true)
    pairs, _ = table.matches(thresh)
    return matching_from_record(table.record(), pairs, thresh, criterion, simple=True)


def instance_metrics(seg, gt, names: Optional[Iterable[str]] = None, thresh: float = 0.5) -> dict:
    """The entries the reference's evaluation writes (evaluation/metric_execution.py:78-163) for the metric names asked for, from ONE
    table: adapted_rand -> adapted_rand_error / _precision / _recall; voi -> voi_split / voi_merge / voi_total; instance_accuracy;
    instance_accuracy_detail -> instance_accuracy_detail and instance_precision_detail / _recall_detail / _f1_detail."""
    names = list(INSTANCE_METRIC_NAMES if names is None else names)
    out = {}
    if not any(n in INSTANCE_METRIC_NAMES for n in names):
        return out
    _same_shape(seg, gt)
    table = _table(seg, gt)
    rec = table.record()
    if "adapted_rand" in names:
        are, precision, recall = adapted_rand_from_record(rec, True)
        out.update(adapted_rand_error=float(are), adapted_rand_precision=float(precision), adapted_rand_recall=float(recall))
    if "voi" in names:
        split, merge = voi_from_record(rec)
        out.update(voi_split=split, voi_merge=merge, voi_total=split + merge)
    if "instance_accuracy" in names or "instance_accuracy_detail" in names:
        pairs, _ = table.matches(float(thresh))
        if "instance_accuracy" in names:
            out["instance_accuracy"] = matching_from_record(rec, pairs, thresh)["accuracy"]
        if "instance_accuracy_detail" in names:
            simple = matching_from_record(rec, pairs, thresh, simple=True)
            out.update(instance_accuracy_detail=simple["accuracy"], instance_precision_detail=simple["precision"],
                       instance_recall_detail=simple["recall"], instance_f1_detail=simple["f1"])
    return out

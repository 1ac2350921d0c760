"""From the integer record of a label-pair table (hip_ops.PairTable.record) and its match list to the reference's numbers.  Plain host
functions on Python ints and numpy scalars: no device, no tensors.

The record's cells (include/pytc_hip.h pytc_pair_table_build): N, N1, S_A, S_B, S_AB, c, n_true, n_pred, pairs, and the two VOI sums
voi_split_fixed / voi_merge_fixed in VOI_FRAC_BITS-bit fixed point."""
from __future__ import annotations

from typing import Mapping

import numpy as np

VOI_FRAC_BITS = 27


def adapted_rand_from_record(rec: Mapping[str, int], all_stats: bool = False):
    """metrics/segmentation_numpy.py:200-213 with the reference's own float64 expressions on its int64 sums, so the result is the
    reference's bit for bit, the nan of a ground truth without foreground included."""
    with np.errstate(all="ignore"):
        n = int(rec["N"])
        c_over_n = np.int64(rec["c"]) / n
        sum_a = np.int64(rec["S_A"])
        sum_b = np.int64(rec["S_B"]) + c_over_n
        sum_ab = np.int64(rec["S_AB"]) + c_over_n
        precision = sum_ab / sum_b
        recall = sum_ab / sum_a
        f_score = 2.0 * precision * recall / (precision + recall)
        are = 1.0 - f_score
    return (are, precision, recall) if all_stats else are


def voi_from_record(rec: Mapping[str, int]):
    """(split, merge) = (H(seg | gt), H(gt | seg)) over the voxels with gt >= 1: the fixed-point sums divided by 2^VOI_FRAC_BITS N1.
    Without ground-truth foreground the reference divides 0 by 0: nan."""
    n1 = int(rec["N1"])
    if n1 == 0:
        return (float("nan"), float("nan"))
    scale = float(1 << VOI_FRAC_BITS)
    return (int(rec["voi_split_fixed"]) / scale / n1, int(rec["voi_merge_fixed"]) / scale / n1)


def maximum_matching_size(pairs: np.ndarray) -> int:
    """The size of a maximum bipartite matching of the (gt id, seg id) pairs that passed the threshold.  The reference's Hungarian cost
    -[score >= thr] - score / (2 n_matched) first maximises the number of passing pairs (the second term sums to at most 0.5), so its
    `tp` is this number; the sparse graph needs no n_true x n_pred matrix."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(pairs) == 0:
        return 0
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_bipartite_matching
    _, rows = np.unique(pairs[:, 0], return_inverse=True)
    _, cols = np.unique(pairs[:, 1], return_inverse=True)
    graph = csr_matrix((np.ones(len(pairs), dtype=np.int8), (rows, cols)), shape=(int(rows.max()) + 1, int(cols.max()) + 1))
    return int((maximum_bipartite_matching(graph, perm_type="column") >= 0).sum())


def _stats(tp: int, n_true: int, n_pred: int, thresh: float, criterion: str) -> dict:
    fp, fn = n_pred - tp, n_true - tp
    return dict(criterion=criterion, thresh=thresh, fp=fp, tp=tp, fn=fn,
                precision=tp / (tp + fp) if tp > 0 else 0, recall=tp / (tp + fn) if tp > 0 else 0,
                accuracy=tp / (tp + fp + fn) if tp > 0 else 0, f1=(2 * tp) / (2 * tp + fp + fn) if tp > 0 else 0,
                n_true=n_true, n_pred=n_pred)


def matching_from_record(rec: Mapping[str, int], pairs: np.ndarray, thresh: float, criterion: str = "iou", simple: bool = False) -> dict:
    """The reference's stats dict (segmentation_numpy.py:727-742 without the matched-score entries, :843-855 for `simple`): tp is the
    number of passing pairs (simple) or the size of their maximum matching."""
    tp = len(np.asarray(pairs).reshape(-1, 2)) if simple else maximum_matching_size(pairs)
    return _stats(int(tp), int(rec["n_true"]), int(rec["n_pred"]), float(thresh), criterion)

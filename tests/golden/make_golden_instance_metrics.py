"""Generate tests/golden/instance_metrics.npz from the REFERENCE's own metric functions (run in the build container only).

    python tests/golden/make_golden_instance_metrics.py

Drives connectomics/metrics/segmentation_numpy.py adapted_rand(all_stats=True), voi, instance_matching and instance_matching_simple
(thresholds 0.3, 0.5, 0.75) through tests/golden/_ref_shim.py on the label pairs of tests/instance_metric_cases.py `fixture_cases()`.

The module imports `skimage.segmentation.relabel_sequential`, and skimage is not installed.  It is used only by the two matching
functions and only to rank the ids, so a numpy stand-in is registered for it: zero stays zero, the other ids present are ranked
ascending to 1 .. K (np.unique), which is what skimage's function returns for its default offset 1; the forward and inverse maps it
also returns are plain arrays here (the reference reads them only with report_matches).

Stored per case: `<name>__gt`, `<name>__seg` (int64), `<name>__are` (are, precision, recall as float64, nan where the reference gives
nan), `<name>__voi` (split, merge), and per threshold t in (30, 50, 75) `<name>__match_t` / `<name>__simple_t` = (tp, fp, fn, n_true,
n_pred) as int64 and `<name>__match_t_ratios` / `<name>__simple_t_ratios` = (precision, recall, accuracy, f1) as float64.  A function
that raises on a case (voi on a ground truth without foreground) is stored as nan.  Data only.

Also written: `minimal_affinity_eval_label.npz`, the test label of tutorials/minimal_affinity_eval.yaml (no reference code involved): a
blocky int32 id volume of 9 x 15 x 11 boxes with the shape of that tutorial's cropped prediction, 36 x 45 x 77, ids up to 2^24 + 40 and
a fifth of the boxes background.
"""
from __future__ import annotations

import sys
import types
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import _ref_shim as S  # noqa: E402
from instance_metric_cases import THRESHOLDS, _blocks, fixture_cases  # noqa: E402


def relabel_sequential(label_field, offset=1):
    ids = np.unique(label_field)
    ids = ids[ids != 0]
    forward = np.zeros(int(label_field.max()) + 1 if label_field.size else 1, dtype=np.int64)
    forward[ids] = np.arange(offset, offset + len(ids))
    inverse = np.concatenate([[0], ids]).astype(np.int64)
    return forward[label_field], forward, inverse


def _reference():
    S.install()
    S._stub_pkg("connectomics.metrics")
    if "skimage" not in sys.modules:
        sk, seg = types.ModuleType("skimage"), types.ModuleType("skimage.segmentation")
        seg.relabel_sequential = relabel_sequential
        sk.segmentation = seg
        sys.modules["skimage"], sys.modules["skimage.segmentation"] = sk, seg
    return S.ref("connectomics.metrics.segmentation_numpy")


def tutorial_label():
    return _blocks(np.random.default_rng(39), (36, 45, 77), (9, 15, 11), 2 ** 24 + 40, zero_every=5).astype(np.int32)


def main():
    np.savez_compressed(HERE / "minimal_affinity_eval_label.npz", label=tutorial_label())
    ref = _reference()
    out = {}
    warnings.simplefilter("ignore")
    for name, (gt, seg) in fixture_cases().items():
        out[f"{name}__gt"], out[f"{name}__seg"] = gt, seg
        with np.errstate(all="ignore"):
            out[f"{name}__are"] = np.asarray(ref.adapted_rand(seg, gt, all_stats=True), dtype=np.float64)
            try:
                out[f"{name}__voi"] = np.asarray(ref.voi(seg, gt), dtype=np.float64)
            except Exception as e:                              # noqa: BLE001 -- recorded as nan, named on the console
                print(name, "voi raised", type(e).__name__, e)
                out[f"{name}__voi"] = np.full(2, np.nan)
        for thr in THRESHOLDS:
            for tag, fn in (("match", ref.instance_matching), ("simple", ref.instance_matching_simple)):
                st = fn(gt, seg, thresh=thr, criterion="iou")
                key = f"{name}__{tag}_{int(round(thr * 100))}"
                out[key] = np.asarray([st[k] for k in ("tp", "fp", "fn", "n_true", "n_pred")], dtype=np.int64)
                out[key + "_ratios"] = np.asarray([st[k] for k in ("precision", "recall", "accuracy", "f1")], dtype=np.float64)
        print(name, gt.shape, "are", out[f"{name}__are"], "voi", out[f"{name}__voi"], "match@50", out[f"{name}__match_50"],
              "simple@50", out[f"{name}__simple_50"])
    np.savez_compressed(HERE / "instance_metrics.npz", **out)
    print("wrote instance_metrics.npz", len(out), "arrays", (HERE / "instance_metrics.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()

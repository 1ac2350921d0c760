"""Generate tests/golden/label_targets.npz from the REFERENCE's own target functions (run in the build container only).

    python tests/golden/make_golden_label_targets.py

Drives connectomics/data/processing/target.py (seg_to_affinity, seg_to_instance_bd, seg_to_binary, seg_to_polarity,
seg_to_eroded_foreground) and segment.py (seg_erosion_instance) through tests/golden/_ref_shim.py on the seeded labels of
tests/label_target_cases.py.  target.py imports cc3d, fastremap and skimage, which this container lacks and none of the six functions
uses: empty stand-in modules are registered for them and for `.flow`.  transforms.py needs MONAI, so the stacking and mask rule of
MultiTaskLabelTransformd is restated here: per target an optional erosion of a label copy (transforms.py:1043-1049), the function's
values as float32 (:1099-1109), for the mask the affinity target's own mask or `_ignore_aware_mask` (:737-751, :1102-1111), channels
concatenated in task order (:1113-1122), a mask only when an affinity task is present (:884-888); the global `erosion` erodes the patch
first (data/augmentation/build.py:323-325).  Also one array set from the reference LossOrchestrator: a PerChannelBCEWithLogitsLoss term
on a 3-channel affinity target with a label_mask.

It also writes minimal_affinity_image.npz / minimal_affinity_label.npz, the small id volume tutorials/minimal_affinity.yaml trains on.

Values are stored as uint8 (they are 0 / 1 / 2), masks as bool, eroded labels as int32.
"""
from __future__ import annotations

import sys
import types
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import _ref_shim as S  # noqa: E402
from label_target_cases import CASES, demo_volume, make_label  # noqa: E402

DEFAULTS = {"binary": {}, "eroded_foreground": {"tsz_h": 2}, "affinity": {"offsets": ["1-0-0", "0-1-0", "0-0-1"]},
            "instance_boundary": {"thickness": 1, "edge_mode": "seg-all", "mode": "3d"}, "polarity": {"exclusive": False}}


def _reference():
    S.install()
    for name in ("cc3d", "fastremap", "skimage", "skimage.morphology"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["skimage.morphology"].binary_dilation = sys.modules["skimage.morphology"].disk = None
    flow = types.ModuleType("connectomics.data.processing.flow")
    flow.seg2d_to_flows = None
    sys.modules["connectomics.data.processing.flow"] = flow
    return S.ref("connectomics.data.processing.target"), S.ref("connectomics.data.processing.segment")


def _ignore_aware_mask(lab, shape):
    if not (lab < 0).any():
        return np.ones(shape, dtype=bool)
    return np.broadcast_to((lab != -1)[None], shape)


def reference_sample(tg, sg, seg, cfg):
    fns = {"binary": tg.seg_to_binary, "eroded_foreground": tg.seg_to_eroded_foreground, "affinity": tg.seg_to_affinity,
           "instance_boundary": tg.seg_to_instance_bd, "polarity": tg.seg_to_polarity}
    seg = seg.astype(np.int64)                               # the reference's `seg.max() + 1` sentinel must not wrap at 2^31 - 1
    if int(cfg.get("erosion", 0) or 0) > 0:
        seg = sg.seg_erosion_instance(seg, int(cfg["erosion"]))
    tasks = [(t, {}) if isinstance(t, str) else (t["name"], dict(t.get("kwargs", {}))) for t in cfg["targets"]]
    use_mask = any(n == "affinity" for n, _ in tasks)
    outputs, masks = [], []
    for name, kwargs in tasks:
        kw = {**DEFAULTS[name], **kwargs}
        own = int(kw.pop("erosion", 0))
        task_label = sg.seg_erosion_instance(seg, own) if own > 0 else seg
        result = fns[name](task_label, **kw)
        if isinstance(result, tg.AffinityTarget):
            outputs.append(np.asarray(result.values, dtype=np.float32))
            masks.append(np.asarray(result.mask))
        else:
            arr = np.asarray(result, dtype=np.float32)
            arr = arr[None] if arr.ndim == 3 else arr
            outputs.append(arr)
            masks.append(_ignore_aware_mask(task_label, arr.shape))
    return np.concatenate(outputs, axis=0), (np.concatenate(masks, axis=0) if use_mask else None)


def _fits(o, shape):
    return all(abs(d) < n for d, n in zip(o, shape))


def check_not_constant(name, k, cfg, values, mask, shape):
    """both 0 and 1 in at least 2 % of the voxels of every channel whose offset fits inside the volume, values and mask alike"""
    from label_target_cases import _offsets
    fits = []
    for t in cfg["targets"]:
        tname, kw = (t, {}) if isinstance(t, str) else (t["name"], t.get("kwargs", {}))
        if tname == "affinity":
            fits += [_fits(o, shape) for o in _offsets(kw)]
        else:
            fits += [True] * (3 if tname == "polarity" and not kw.get("exclusive") else 1)
    assert len(fits) == values.shape[1], (name, len(fits), values.shape)
    for c, ok in enumerate(fits):
        if not ok:
            assert not values[:, c].any() and (mask is None or not mask[:, c].any()), (name, k, c)
            continue
        for what, arr in (("values", values), ("mask", mask)):
            if arr is None:
                continue
            ch = arr[:, c]
            for level in (0, 1):
                frac = float((ch == level).mean())
                assert frac >= 0.02, f"{name}[{k}] channel {c} {what}: level {level} covers {frac:.3%} of the voxels"


def orchestrator_case(out):
    """the reference LossOrchestrator on a PerChannelBCEWithLogitsLoss term over a 3-channel affinity target with a label_mask"""
    ls = S.ref("connectomics.models.losses.losses")
    S._stub_pkg("connectomics.training.losses")
    S._stub_pkg("connectomics.config.pipeline")
    meta = S.ref("connectomics.models.losses.metadata")
    ml = sys.modules["connectomics.models.losses"]
    for n in dir(meta):
        if not n.startswith("_"):
            setattr(ml, n, getattr(meta, n))
    orch = S.ref("connectomics.training.losses.orchestrator")
    terms = [{"function": "PerChannelBCEWithLogitsLoss", "weight": 1.0, "kwargs": {}}]
    targets = [{"name": "affinity", "kwargs": {"affinity_mode": "deepem"}}]
    cfg = NS(model=NS(loss=NS(deep_supervision=False, deep_supervision_weights=[1.0], deep_supervision_clamp_min=-20.0,
                              deep_supervision_clamp_max=20.0, losses=terms, loss_balancing=None),
                      primary_head=None, heads=None, out_channels=3),
             data=NS(label_transform=NS(targets=targets, stack_outputs=True)))
    o = orch.LossOrchestrator(cfg, torch.nn.ModuleList([ls.PerChannelBCEWithLogitsLoss()]), [1.0], enable_nan_detection=True,
                              debug_on_nan=False, resolve_affinity_mode_fn=lambda c: "deepem")
    g = torch.Generator().manual_seed(9190)
    logits = torch.randn(2, 3, 4, 6, 7, generator=g) * 9.0
    tg, sg = _reference()
    rng = np.random.default_rng(9191)
    lab = np.repeat(np.repeat(rng.integers(0, 4, size=(2, 4, 3, 4)), 2, axis=2), 2, axis=3)[:, :, :6, :7].astype(np.int64)
    lab[:, :, :, 6] = -1
    pairs = [reference_sample(tg, sg, s, {"targets": targets}) for s in lab]
    labels = torch.from_numpy(np.stack([v for v, _ in pairs]))
    lmask = torch.from_numpy(np.stack([m for _, m in pairs]).copy())
    x = logits.clone().requires_grad_(True)
    try:
        total, _ = o.compute_standard_loss(x, labels, stage="train", mask=None, target_mask=lmask)
    except TypeError:
        total, _ = o.compute_standard_loss(x, labels, stage="train", mask=None, label_mask=lmask)
    total.backward()
    out["orch__logits"], out["orch__labels"], out["orch__label_mask"] = logits.numpy(), labels.numpy().astype(np.uint8), lmask.numpy()
    out["orch__total"] = total.detach().numpy().astype(np.float64)
    out["orch__grad"] = x.grad.numpy()
    print("orch", float(total.detach()))


def main():
    tg, sg = _reference()
    out = {}
    for name in sorted(CASES):
        case = CASES[name]
        label = make_label(name)
        assert label.shape == (case["batch"],) + tuple(case["shape"]) and label.dtype == np.int32, (name, label.shape)
        out[f"{name}__label"] = label
        for half in case["erode"]:
            arg = half[1] if (half[0] == 0 and half[1] == half[2]) else half      # the scalar form where it says the same
            er = np.stack([sg.seg_erosion_instance(s.astype(np.int64), arg) for s in label])
            assert er.min() >= -2 ** 31 and er.max() <= 2 ** 31 - 1
            out[f"{name}__erode_{half[0]}_{half[1]}_{half[2]}"] = er.astype(np.int32)
        for k, cfg in enumerate(case["configs"]):
            pairs = [reference_sample(tg, sg, s, cfg) for s in label]
            values = np.stack([v for v, _ in pairs])
            mask = np.stack([m for _, m in pairs]) if pairs[0][1] is not None else None
            assert set(np.unique(values)) <= {0.0, 1.0, 2.0}
            if name != "big_ids":
                check_not_constant(name, k, cfg, values, mask, case["shape"])
            out[f"{name}__{k}__values"] = values.astype(np.uint8)
            if mask is not None:
                out[f"{name}__{k}__mask"] = mask.astype(bool)
            print(name, k, values.shape, "mask" if mask is not None else "no mask")
    orchestrator_case(out)
    # the volume tutorials/minimal_affinity.yaml trains on (no reference code involved: tests/label_target_cases.py demo_volume)
    image, lab = demo_volume()
    np.savez_compressed(HERE / "minimal_affinity_image.npz", image=image)
    np.savez_compressed(HERE / "minimal_affinity_label.npz", label=lab)
    np.savez_compressed(HERE / "label_targets.npz", **out)
    print("wrote label_targets.npz", len(out), "arrays", (HERE / "label_targets.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()

"""Generate tests/golden/augment.npz from the REFERENCE's own augmentation code (run in the build container only).

    python tests/golden/make_golden_augment.py

Drives, through tests/golden/_ref_shim.py, on the seeded cases of tests/augment_cases.py:
  * the pure functions of connectomics/data/augmentation/augment_ops.py with explicit parameters (PURE_CASES);
  * the nine transform classes of transforms.py that the device plan follows draw for draw (CLASS_CASES), each with a seeded
    numpy RandomState.
augment_ops.py imports cv2 and transforms.py imports torchvision and monai, which this container lacks and none of the code driven here
uses: empty stand-in modules are registered for them, and a minimal MapTransform / RandomizableTransform pair written here (keys,
key_iterator, R, set_random_state, prob, _do_transform) stands in for MONAI's base classes.

Per case the file holds the output (`<case>__out`, for the geometric classes also `<case>__label_out`) and, per class case, the value
the class's generator draws next after each call (`<case>__next`: every draw the class takes, also one that no longer changes the
output, moves it); inputs are regenerated from their seeds by tests/augment_cases.py, and a few are stored (`<case>__in`) so that a
drifting generator shows.
"""
from __future__ import annotations

import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))
import _ref_shim as S  # noqa: E402
import augment_cases as X  # noqa: E402


class MapTransform:
    def __init__(self, keys, allow_missing_keys=False):
        self.keys = (keys,) if isinstance(keys, str) else tuple(keys)
        self.allow_missing_keys = allow_missing_keys

    def key_iterator(self, data):
        for key in self.keys:
            if key in data:
                yield key
            elif not self.allow_missing_keys:
                raise KeyError(key)


class RandomizableTransform:
    def __init__(self, prob=1.0, do_transform=True):
        self._do_transform = do_transform
        self.prob = min(max(prob, 0.0), 1.0)
        self.R = np.random.RandomState()

    def set_random_state(self, seed=None, state=None):
        self.R = state if state is not None else np.random.RandomState(seed)
        return self

    def randomize(self, data=None):
        self._do_transform = self.R.rand() < self.prob


def _reference():
    S.install()
    sys.modules.pop("connectomics.data.augmentation.augment_ops", None)          # the shim's stand-in: the real module is wanted here
    for name in ("cv2", "torchvision", "torchvision.transforms", "torchvision.transforms.functional", "monai", "monai.config",
                 "monai.transforms"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["torchvision.transforms"].functional = sys.modules["torchvision.transforms.functional"]
    sys.modules["monai.config"].KeysCollection = object
    sys.modules["monai.transforms"].MapTransform = MapTransform
    sys.modules["monai.transforms"].RandomizableTransform = RandomizableTransform
    return S.ref("connectomics.data.augmentation.augment_ops"), S.ref("connectomics.data.augmentation.transforms")


def class_kwargs(block, cfg):
    """the constructor arguments `_build_augmentations` passes for a block"""
    if block == "intensity":
        return {"prob": cfg["mul_add_prob"], "mul_range": cfg["mul_range"], "add_range": cfg["add_range"]}
    return {k: v for k, v in cfg.items()}


def main():
    ops, tf = _reference()
    out = {}
    for name, case in X.PURE_CASES.items():
        vol = (X.make_ids if case["ids"] else X.make_image)(case["shape"], case["seed"])
        kwargs = dict(case["kwargs"])
        for key in ("indices", "permutation", "neighbor_directions"):
            if key in kwargs:
                kwargs[key] = np.asarray(kwargs[key], dtype=np.int64)
        if "shifts" in kwargs:
            kwargs["shifts"] = [tuple(s) for s in kwargs["shifts"]]
        if "rotate_ks" in kwargs:
            kwargs["rotate_ks"] = tuple(kwargs["rotate_ks"])
        res = np.ascontiguousarray(getattr(ops, case["fn"])(vol.copy(), **kwargs))
        assert res.dtype == vol.dtype and res.shape == vol.shape, (name, res.dtype, res.shape)
        out[f"fn__{name}__out"] = res
    out["fn__lost_interpolate__in"] = X.make_image(X.PURE_CASES["lost_interpolate"]["shape"], X.PURE_CASES["lost_interpolate"]["seed"])
    for cls_name, cases in X.CLASS_CASES.items():
        cls = getattr(tf, cls_name)
        changed = same = 0
        for i, case in enumerate(cases):
            keys = ["image", "label"] if case.get("label") else ["image"]
            alias = {"slice_shift_z": tf.RandSliceShiftZd, "slice_drop_z": tf.RandSliceDropZd}.get(case["block"], cls)
            following = []
            for seed in case["seeds"]:
                image, label = X.class_case_arrays(cls_name, i, seed)
                t = alias(keys=keys, **class_kwargs(case["block"], case["cfg"]))
                t.set_random_state(state=np.random.RandomState(seed))
                data = {"image": image.copy()}
                if label is not None:
                    data["label"] = label.copy()
                res = t(data)
                img = np.ascontiguousarray(res["image"])
                assert img.dtype == np.float32 and img.shape == image.shape, (cls_name, i, seed, img.dtype, img.shape)
                out[f"cls__{cls_name}__{i}__{seed}__out"] = img
                if label is not None:
                    out[f"cls__{cls_name}__{i}__{seed}__label_out"] = np.ascontiguousarray(res["label"])
                if np.array_equal(img.view(np.int32), image.view(np.int32)):
                    same += 1
                else:
                    changed += 1
                following.append(int(t.R.randint(2 ** 31 - 1)))     # where the class left its generator: the next draw
            out[f"cls__{cls_name}__{i}__next"] = np.array(following, dtype=np.int64)
        assert changed >= 3 and same >= 1, f"{cls_name}: {changed} changed, {same} unchanged outputs: the seeds must show both"
        print(cls_name, "changed", changed, "unchanged", same)
    image, _ = X.class_case_arrays("RandLostSectiond", 1, X.CLASS_CASES["RandLostSectiond"][1]["seeds"][0])
    out["cls__RandLostSectiond__1__in"] = image
    np.savez_compressed(HERE / "augment.npz", **out)
    print("wrote augment.npz", len(out), "arrays", (HERE / "augment.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()

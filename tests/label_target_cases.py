"""Seeded cases of the device label-target transform (tests/test_host_label_targets.py, tests/test_gpu_label_targets.py,
tests/golden/make_golden_label_targets.py) and a numpy model of it in GATHER form: every output voxel looks up the voxels it depends
on, as include/pytc_hip.h states the kernels' arithmetic -- not the slice-and-assign form of the reference's functions, which the
fixture tests/golden/label_targets.npz records.

Labels are blocky instance maps: a coarse grid of ids drawn from a small pool, blown up by a block size and REPEATED over the volume
(so that long offsets meet equal ids), with background cells, a background gap and a slab of -1 ("unlabeled").  Voxel noise would be
no use: the erosion erases it entirely.
"""
from __future__ import annotations

import numpy as np

AFF12 = ["0-0-1", "0-1-0", "1-0-0", "2-0-0", "3-0-0", "4-0-0", "0-0-3", "0-0-9", "0-0-27", "0-3-0", "0-9-0", "0-27-0"]
SIGNED = [[-1, 2, 0], [0, 0, 0], [3, -3, 1], [0, 0, -5]]
BIG_A, BIG_B, BIG_C = 2 ** 24, 1 + 2 ** 24, 2 ** 31 - 1          # float32 reads the first two as one id and the third as 2^31


def _aff(**kw):
    return {"name": "affinity", "kwargs": kw}


# name -> batch, shape, how the label is made, the `data.label_transform` configs it is run under, the half-sizes of the erosion
# kernel run on it alone
CASES = {
    "aff12_erosion1": dict(batch=2, shape=(5, 31, 33), label=dict(block=(2, 9, 9), coarse=(2, 3, 3), pool=(0, 1, 2, 3), seed=9101,
                                                                  gap=("y", 13, 1), slab=("x", 31, 2)),
                           configs=[{"erosion": 1, "targets": [_aff(offsets=AFF12, affinity_mode="deepem")]}],
                           erode=[(0, 1, 1), (1, 1, 1), (10, 10, 4)]),
    "banis_long_range": dict(batch=1, shape=(12, 9, 14), label=dict(block=(5, 5, 5), coarse=(2, 2, 2), pool=(0, 1, 2, 2), seed=9102,
                                                                    gap=("z", 5, 1), slab=("y", 8, 1)),
                             configs=[{"targets": [_aff(long_range=10, affinity_mode="banis")]}],
                             erode=[(0, 1, 1), (2, 0, 3)]),
    "signed_diagonal": dict(batch=2, shape=(4, 7, 6), label=dict(block=(3, 3, 5), coarse=(1, 2, 1), pool=(1, 2, 2, 0), seed=9203,
                                                                 gap=None, slab=("rows", 6, 1)),
                            configs=[{"targets": [_aff(offsets=SIGNED, affinity_mode="deepem")]},
                                     {"targets": [_aff(offsets=SIGNED, affinity_mode="banis")]}],
                            erode=[(0, 1, 1), (4, 3, 0)]),
    "depth1": dict(batch=2, shape=(1, 17, 19), label=dict(block=(1, 6, 6), coarse=(1, 3, 4), pool=(0, 1, 2, 3, 4, 5), seed=9104,
                                                          gap=("y", 8, 1), slab=("x", 17, 2)),
                   configs=[{"targets": [_aff(affinity_mode="deepem"),
                                         {"name": "instance_boundary", "kwargs": {"mode": "2d"}}, "binary"]}],
                   erode=[(0, 1, 1), (3, 2, 2)]),
    "no_affinity": dict(batch=1, shape=(3, 10, 11), label=dict(block=(2, 4, 4), coarse=(2, 3, 3), pool=(0, 1, 2, 3, 4, 5, 6), seed=9105,
                                                               gap=("y", 5, 1), slab=("x", 10, 1)),
                        configs=[{"targets": ["binary"]
                                  + [{"name": "instance_boundary", "kwargs": {"edge_mode": e, "mode": m}}
                                     for m in ("3d", "2d") for e in ("all", "seg-all", "seg-no-bg")]
                                  + ["polarity", {"name": "polarity", "kwargs": {"exclusive": True}}]}],
                        erode=[(0, 1, 1), (1, 0, 0)]),
    "multi_erosion": dict(batch=2, shape=(6, 20, 21), label=dict(block=(6, 7, 7), coarse=(1, 3, 3), pool=(3, 5, 2, 4, 3, 5, 0), seed=9106,
                                                                 gap=("y", 10, 1), slab=("x", 20, 1)),
                          configs=[{"targets": [_aff(affinity_mode="deepem", erosion=2),
                                                "eroded_foreground",
                                                {"name": "eroded_foreground", "kwargs": {"tsz_h": [2, 2, 1]}},
                                                {"name": "binary", "kwargs": {"segment_id": [3, 5]}},
                                                _aff(affinity_mode="deepem", semantic=True)]}],
                          erode=[(0, 2, 2), (2, 2, 1)]),
    "big_ids": dict(batch=1, shape=(2, 3, 9), label="big_ids",
                    configs=[{"targets": [_aff(affinity_mode="deepem"), "binary", "polarity"]}],
                    erode=[(0, 1, 1), (1, 1, 1)]),
}


def make_label(name: str) -> np.ndarray:
    """int32 (B, D, H, W) instance ids of a case."""
    case = CASES[name]
    B, shape = case["batch"], case["shape"]
    if case["label"] == "big_ids":
        row = np.array([1, 1, BIG_A, BIG_B, BIG_B, BIG_C, BIG_C, 0, -1], dtype=np.int64)
        lab = np.stack([np.stack([np.roll(row, y + 2 * z) for y in range(shape[1])]) for z in range(shape[0])])
        return lab[None].astype(np.int32)
    spec = case["label"]
    rng = np.random.default_rng(spec["seed"])
    out = []
    for _ in range(B):
        coarse = rng.choice(np.asarray(spec["pool"]), size=spec["coarse"])
        cell = coarse
        for ax, b in enumerate(spec["block"]):
            cell = np.repeat(cell, b, axis=ax)
        reps = [-(-s // c) for s, c in zip(shape, cell.shape)]
        lab = np.tile(cell, reps)[:shape[0], :shape[1], :shape[2]].copy()
        for what, fill in ((spec["gap"], 0), (spec["slab"], -1)):
            if what is None:
                continue
            axis, at, width = what
            if axis == "rows":                               # whole x-rows of the first plane
                lab[0, at:at + width, :] = fill
            else:
                sl = [slice(None)] * 3
                sl["zyx".index(axis)] = slice(at, at + width)
                lab[tuple(sl)] = fill
        out.append(lab)
    return np.stack(out).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- the numpy model
def _gather(seg: np.ndarray, o, fill):
    """(the id at p + o for every voxel p of one (D, H, W) sample, `fill` beyond the volume;  whether p + o lies inside)"""
    out = np.full(seg.shape, fill, dtype=seg.dtype)
    inside = np.zeros(seg.shape, dtype=bool)
    src, dst = [], []
    for n, d in zip(seg.shape, o):
        if abs(d) >= n:
            return out, inside
        dst.append(slice(max(0, -d), n - max(0, d)))
        src.append(slice(max(0, d), n - max(0, -d)))
    out[tuple(dst)] = seg[tuple(src)]
    inside[tuple(dst)] = True
    return out, inside


def model_erode(seg: np.ndarray, half) -> np.ndarray:
    """(D, H, W): keep a voxel where it is negative or its clipped box window holds exactly one distinct positive id."""
    seg = seg.astype(np.int64)
    big = np.iinfo(np.int64).max
    M = np.full(seg.shape, np.iinfo(np.int64).min)
    m = np.full(seg.shape, big)
    for dz in range(-half[0], half[0] + 1):
        for dy in range(-half[1], half[1] + 1):
            for dx in range(-half[2], half[2] + 1):
                v, inside = _gather(seg, (dz, dy, dx), 0)
                M = np.where(inside, np.maximum(M, v), M)
                m = np.where(inside & (v > 0), np.minimum(m, v), m)
    keep = (seg < 0) | ((M > 0) & (M == m))
    return np.where(keep, seg, 0).astype(np.int32)


def _half(tsz_h):
    return (0, int(tsz_h), int(tsz_h)) if np.isscalar(tsz_h) else tuple(int(v) for v in tsz_h)


def _offsets(kw):
    if kw.get("long_range") is not None:
        r = int(kw["long_range"])
        return [(1, 0, 0), (0, 1, 0), (0, 0, 1), (r, 0, 0), (0, r, 0), (0, 0, r)]
    offs = kw.get("offsets") or ["1-0-0", "0-1-0", "0-0-1"]
    return [tuple(int(v) for v in (o.split("-") if isinstance(o, str) else o)) for o in offs]


def _edge(a, b, mode):
    d = a != b
    if mode == "seg-all":
        d &= (a > 0) | (b > 0)
    elif mode == "seg-no-bg":
        d &= (a > 0) & (b > 0)
    return d


def model_sample(seg: np.ndarray, cfg: dict):
    """One (D, H, W) int32 sample under a `label_transform` config -> (values float32 (C, D, H, W), mask bool (C, D, H, W) or None)."""
    if int(cfg.get("erosion", 0) or 0) > 0:
        seg = model_erode(seg, _half(int(cfg["erosion"])))
    tasks = [(t, {}) if isinstance(t, str) else (t["name"], dict(t.get("kwargs", {}))) for t in cfg["targets"]]
    use_mask = any(n == "affinity" for n, _ in tasks)
    values, masks = [], []
    for name, kw in tasks:
        s = seg
        own = int(kw.pop("erosion", 0))
        if own > 0:
            s = model_erode(seg, _half(own))
        plain = s != -1
        if name == "affinity":
            banis = kw["affinity_mode"] == "banis"
            t = np.where(s > 0, 1, s) if kw.get("semantic") else s
            for o in _offsets(kw):
                other, inside = _gather(t, o if banis else tuple(-v for v in o), 0)      # banis: q = p + o; deepem: q = p - o
                values.append(inside & (t == other) & (t > 0))
                masks.append(inside & (t != -1) & (other != -1))
        elif name == "binary":
            ids = kw.get("segment_id") or []
            values.append(np.isin(s, ids) if ids else s > 0)
            masks.append(plain)
        elif name == "eroded_foreground":
            values.append(model_erode(s, _half(kw.get("tsz_h", 2))) > 0)
            masks.append(plain)
        elif name == "instance_boundary":
            mode, planar = kw.get("edge_mode", "seg-all"), kw.get("mode", "3d") != "3d"
            hit = np.zeros(s.shape, dtype=bool)
            for axis in ((1, 2) if planar else (0, 1, 2)):
                for step in (-1, 1):
                    o = [0, 0, 0]
                    o[axis] = step
                    q, inside = _gather(s, o, 0)
                    hit |= inside & _edge(s, q, mode)
            values.append(hit)
            masks.append(plain)
        elif name == "polarity":
            pos, neg = (s > 0) & (s % 2 == 1), (s > 0) & (s % 2 == 0)
            if kw.get("exclusive"):
                values.append(pos.astype(np.float32) + 2 * neg.astype(np.float32))
                masks.append(plain)
            else:
                values += [pos, neg, s > 0]
                masks += [plain] * 3
        else:
            raise KeyError(name)
    return np.stack([v.astype(np.float32) for v in values]), (np.stack(masks) if use_mask else None)


def model_batch(label: np.ndarray, cfg: dict):
    """(B, D, H, W) -> (values (B, C, D, H, W) float32, mask bool or None)."""
    outs = [model_sample(lab, cfg) for lab in label]
    return np.stack([v for v, _ in outs]), (np.stack([m for _, m in outs]) if outs[0][1] is not None else None)


# ---------------------------------------------------------------------------------------------------------------- a training volume
def demo_volume(seed: int = 9400, shape=(40, 48, 48), block=(8, 12, 12)):
    """(image uint8, label int32) of one small training volume: every coarse cell is an instance of its own (some are background),
    one id lies above 2^24, one slab is unlabeled; the image is the foreground plus noise."""
    rng = np.random.default_rng(seed)
    coarse = tuple(-(-s // b) for s, b in zip(shape, block))
    ids = rng.permutation(int(np.prod(coarse))).reshape(coarse).astype(np.int64) + 1
    ids[rng.random(coarse) < 0.2] = 0
    ids[ids == ids.max()] = BIG_B + 4
    lab = ids
    for ax, b in enumerate(block):
        lab = np.repeat(lab, b, axis=ax)
    lab = lab[:shape[0], :shape[1], :shape[2]].copy()
    lab[:, :, -2:] = -1
    image = np.clip((lab > 0) * 110 + rng.normal(70, 25, size=shape), 0, 255).astype(np.uint8)
    return image, lab.astype(np.int32)

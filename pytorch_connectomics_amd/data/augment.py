"""`data.augmentation` on the device: the flips, quarter turns and axis permutations of a training batch and the EM section defects
of its image, as the reference's augmentation chain applies them on CPU workers (data/augmentation/build.py:741-1000 `_build_augmentations`,
transforms.py, augment_ops.py), by two HIP kernels (csrc/augment_kernels.hip).

    plan = AugmentationPlan.from_config(cfg.data.augmentation, seed=cfg.system.seed + rank)
    if plan.enabled:
        batch = plan(batch)                # image fp32 (N, C, D, H, W); label int32 (N, D, H, W) ids or fp32 (N, 1, D, H, W); optional mask

Per sample the host draws every enabled block's random numbers (one `numpy.random.RandomState` per block, apart from the sampler's
generator) and turns them into two small tables: a signed axis permutation (the geometric blocks composed, one of 48) for image, label
and mask, and a list of op rows (FILL / MOVE / COPY_SECTION / MULADD) for the image.  Both travel to the device in one copy from a pinned
buffer on the current stream; one gather launch per tensor and one defect launch per batch apply them.  Nothing synchronises.

Built, in the reference's build order: axis_permute, rotate90_all, flip, rotate (geometric; axis_permute and rotate90_all act on cubic
patches only, as the reference classes do); slice_drop, slice_shift, intensity (banis_style mul / add, or the shift_intensity term),
slice_shift_z, slice_drop_z, lost_section, misalignment, missing_section, missing_parts (image only), defect_mutex.  Refused by name:
affine, elastic, motion_blur, cut_noise, cut_blur, stripe, mixup, copy_paste, a rotate_ratio above 0 (a warp), Gaussian noise and
contrast (device random numbers and a reduction), 2-D training, more than 4 image channels.

Draw order.  For the nine classes of the reference's own transforms.py (RandAxisPermuted, RandRotate90Alld, RandSliceDropd,
RandSliceShiftd, RandMulAddIntensityd, RandMisAlignmentd, RandMissingSectiond, RandLostSectiond, RandMissingPartsd) the draws follow
the class call for call (the same RandomState methods with the same arguments in the same order, for one (C, D, H, W) sample), so a
block seeded like the class yields the class's output.  `flip`, `rotate`, the shift_intensity term and the defect_mutex pick are
MONAI classes in the reference (RandFlipd, RandRotate90d, RandShiftIntensityd, OneOf); their draw order here is this project's own:
flip: one `rand() < prob` per listed axis, in order; rotate: `rand() < prob`, then `randint(3) + 1` quarter turns; shift_intensity:
`rand() < prob`, then `uniform(-offset, offset)`; defect_mutex: `randint(number of enabled defects)`.
"""
from __future__ import annotations

import copy
import zlib
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _native as nat

GEOMETRIC_BLOCKS = ("axis_permute", "rotate90_all", "flip", "rotate")
IMAGE_BLOCKS = ("slice_drop", "slice_shift", "intensity")
DEFECT_BLOCKS = ("slice_shift_z", "slice_drop_z", "lost_section", "misalignment", "missing_section", "missing_parts")     # build order
BUILT_BLOCKS = GEOMETRIC_BLOCKS + IMAGE_BLOCKS + DEFECT_BLOCKS
REFUSED_BLOCKS = ("affine", "elastic", "motion_blur", "cut_noise", "cut_blur", "stripe", "mixup", "copy_paste")
LOST_SECTION_MODES = ("previous", "next", "random_neighbor", "interpolate")
IDENTITY = (0, 1, 2)

# the reference schema's defaults for the built blocks (connectomics/config/schema/data.py; tests/golden/config_defaults.json)
DEFAULTS: Dict[str, Dict[str, Any]] = {
    "axis_permute": {"enabled": False, "prob": 1.0, "include_identity": True},
    "rotate90_all": {"enabled": False, "prob": 1.0, "include_identity": True},
    "flip": {"enabled": False, "prob": 0.5, "spatial_axis": [0, 1, 2]},
    "rotate": {"enabled": False, "prob": 0.5, "spatial_axes": [1, 2]},
    "slice_drop": {"enabled": False, "prob": 0.0, "slice_prob": 0.05, "spatial_axis": [0, 1, 2], "fill_value": 0.0,
                   "preserve_boundaries": False},
    "slice_shift": {"enabled": False, "prob": 0.0, "slice_prob": 0.05, "shift_magnitude": 10, "spatial_axis": [0, 1, 2], "wrap": True},
    "intensity": {"enabled": False, "banis_style": False, "mul_add_prob": 0.0, "mul_range": [0.9, 1.1], "add_range": [-0.1, 0.1],
                  "gaussian_noise_prob": 0.5, "gaussian_noise_std": 0.1, "shift_intensity_prob": 0.5, "shift_intensity_offset": 0.1,
                  "contrast_prob": 0.5, "contrast_range": [0.9, 1.1]},
    "slice_shift_z": {"enabled": False, "prob": 0.0, "displacement": 16, "rotate_ratio": 0.0},
    "misalignment": {"enabled": False, "prob": 0.0, "displacement": 16, "rotate_ratio": 0.0},
    "slice_drop_z": {"enabled": False, "prob": 0.0, "num_sections": 2, "full_section_prob": 0.5, "partial_ratio_range": [0.25, 0.75],
                     "fill_value_range": [0.0, 1.0]},
    "missing_section": {"enabled": False, "prob": 0.0, "num_sections": 2, "full_section_prob": 0.5, "partial_ratio_range": [0.25, 0.75],
                        "fill_value_range": [0.0, 1.0]},
    "lost_section": {"enabled": False, "prob": 0.0, "num_sections": 1, "mode": "random_neighbor"},
    "missing_parts": {"enabled": False, "prob": 0.0, "hole_range": [8, 32]},
}

Row = Tuple[int, ...]
SignedPerm = Tuple[int, int, int]


def _plain(v: Any) -> Any:
    """config nodes (namespaces, mappings, lists) as plain Python values"""
    if isinstance(v, (str, bytes)) or v is None:
        return v
    if hasattr(v, "items"):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if hasattr(v, "__dict__") and not isinstance(v, (int, float, bool)):
        return {k: _plain(x) for k, x in vars(v).items()}
    return v


def _f32_bits(x: float) -> int:
    """A Python float as numpy rounds it into a float32 array (NEP 50: the scalar takes the array's type), as int32 bits."""
    return int(np.array([x], dtype=np.float64).astype(np.float32).view(np.int32)[0])


# ------------------------------------------------------------------------------------------------- signed permutations
def compose(first: SignedPerm, then: SignedPerm) -> SignedPerm:
    """The signed permutation of applying `first` and then `then`.  Entry v of output axis a names input axis s = v if v >= 0 else
    -1 - v, read backwards when v < 0 (include/pytc_hip.h pytc_augment_permute)."""
    out = []
    for v in then:
        s, f = (v, False) if v >= 0 else (-1 - v, True)
        w = first[s]
        s1, f1 = (w, False) if w >= 0 else (-1 - w, True)
        out.append(-1 - s1 if f != f1 else s1)
    return tuple(out)


def transpose_perm(axes: Sequence[int]) -> SignedPerm:
    """numpy.transpose(x, axes) of the three spatial axes"""
    return tuple(int(a) for a in axes)


def flip_perm(axis: int) -> SignedPerm:
    """numpy.flip(x, axis)"""
    return tuple(-1 - a if a == axis else a for a in range(3))


def rot90_perm(k: int, axes: Tuple[int, int]) -> SignedPerm:
    """numpy.rot90(x, k, axes) on spatial axes: k quarter turns from axes[0] towards axes[1]"""
    a0, a1 = axes
    swap = [0, 1, 2]
    swap[a0], swap[a1] = a1, a0
    k %= 4
    if k == 0:
        return IDENTITY
    if k == 1:                                               # transpose(flip(x, a1))
        return compose(flip_perm(a1), transpose_perm(swap))
    if k == 2:
        return compose(flip_perm(a0), flip_perm(a1))
    return compose(transpose_perm(swap), flip_perm(a1))      # flip(transpose(x), a1)


def rotate90_all_perm(ks: Sequence[int]) -> SignedPerm:
    """augment_ops.apply_rotate90_all: quarter turns in the planes (x, y), (x, z), (y, z), in that order"""
    p = IDENTITY
    for k, axes in zip(ks, ((2, 1), (2, 0), (1, 0))):
        p = compose(p, rot90_perm(int(k), axes))
    return p


def moves_axes(perm: SignedPerm) -> bool:
    return tuple(v if v >= 0 else -1 - v for v in perm) != IDENTITY


def check_signed_perm(perm: Sequence[int], dims: Sequence[int]) -> None:
    src = [int(v) if v >= 0 else -1 - int(v) for v in perm]
    if len(src) != 3 or sorted(src) != [0, 1, 2]:
        raise ValueError(f"{tuple(perm)} is not a signed permutation of the three spatial axes")
    for a, s in enumerate(src):
        if dims[a] != dims[s]:
            raise ValueError(f"permutation {tuple(perm)} moves axis {s} (length {dims[s]}) onto axis {a} (length {dims[a]}) of a "
                             f"{tuple(dims)} patch: the batch shape would change")


# ------------------------------------------------------------------------------------------------- op rows
def fill_row(box: Sequence[int], value: float, dims: Sequence[int]) -> Row:
    """FILL: box = (z0, z1, y0, y1, x0, x1), clipped to the volume as numpy clips a slice"""
    b = []
    for a in range(3):
        lo, hi = max(0, min(int(box[2 * a]), dims[a])), max(0, min(int(box[2 * a + 1]), dims[a]))
        b += [lo, max(lo, hi)]
    return (nat.AUG_FILL, 0, *b, _f32_bits(value), 0)


def move_row(axis: int, lo: int, hi: int, du: int, dv: int, wrap: bool) -> Row:
    """MOVE: slab lo <= c < hi along `axis`, shifted by (du, dv) along its two other axes in ascending order"""
    return (nat.AUG_MOVE, 0, int(axis), int(lo), int(hi), int(du), int(dv), int(bool(wrap)), 0, 0)


def copy_row(z: int, mode: int, group: int) -> Row:
    """COPY_SECTION: section z from z + mode (mode -1 / +1) or the mean of both (mode 0); rows of a group read the group's input"""
    return (nat.AUG_COPY_SECTION, int(group), int(z), int(mode), 0, 0, 0, 0, 0, 0)


def muladd_row(mul: float, add: float) -> Row:
    return (nat.AUG_MULADD, 0, _f32_bits(mul), _f32_bits(add), 0, 0, 0, 0, 0, 0)


def check_rows(rows: Sequence[Row], dims: Sequence[int]) -> None:
    """What the launch checks on its host copy, raised here before anything is uploaded."""
    if len(rows) > nat.AUG_MAX_OPS:
        raise NotImplementedError(f"{len(rows)} image ops for one sample: one launch walks at most {nat.AUG_MAX_OPS} per sample")
    mean_groups = set()
    for k, r in enumerate(rows):
        if len(r) != nat.AUG_ROW:
            raise ValueError(f"op row {k} has {len(r)} entries, not {nat.AUG_ROW}")
        kind, group, p = r[0], r[1], r[2:]
        if kind == nat.AUG_FILL:
            if any(not (0 <= p[2 * a] <= p[2 * a + 1] <= dims[a]) for a in range(3)):
                raise ValueError(f"op row {k}: fill box {p[:6]} outside a {tuple(dims)} volume")
        elif kind == nat.AUG_MOVE:
            if not (0 <= p[0] <= 2) or not (0 <= p[1] <= p[2] <= dims[p[0]]) or p[5] not in (0, 1) or max(abs(p[3]), abs(p[4])) >= 2 ** 30:
                raise ValueError(f"op row {k}: move {p[:6]} outside a {tuple(dims)} volume")
        elif kind == nat.AUG_COPY_SECTION:
            if not (1 <= p[0] <= dims[0] - 2) or p[1] not in (-1, 0, 1):
                raise ValueError(f"op row {k}: section copy {p[:2]} in a volume of depth {dims[0]}")
            if p[1] == 0:
                mean_groups.add(group if group else ("row", k))
        elif kind != nat.AUG_MULADD:
            raise ValueError(f"op row {k}: unknown op kind {kind}")
    if len(mean_groups) > 1:
        raise NotImplementedError("interpolated sections in more than one group: one launch evaluates one level of means")


# ------------------------------------------------------------------------------------------------- settings read once, at plan time
def _axis_candidates(block: str, value: Any) -> np.ndarray:
    """`spatial_axis` of slice_drop / slice_shift as the int64 array of axes a draw picks from: a keyword for all three, one axis, or
    a list.  With one candidate nothing is drawn; with more, one `R.choice` of this very array (the reference's draw)."""
    if isinstance(value, str):
        if value not in ("random", "all", "any"):
            raise ValueError(f"data.augmentation.{block}.spatial_axis {value!r}: a keyword must be 'random', 'all' or 'any'")
        value = [0, 1, 2]
    axes = np.asarray(value, dtype=np.int64).reshape(-1)
    if axes.size == 0 or ((axes < 0) | (axes > 2)).any():
        raise ValueError(f"data.augmentation.{block}.spatial_axis {value}: one or more of the axes 0, 1, 2 of a 3-D patch are needed")
    return axes


def _section_count(block: str, value: Any) -> Tuple[int, int, bool]:
    """`num_sections` as (lowest, highest, drawn): a number is taken as it is, a [min, max] pair costs one `R.randint(lowest,
    highest + 1)` per sample (also when both are equal, as in the reference), an empty list means none."""
    if not isinstance(value, (list, tuple)):
        return int(value), int(value), False
    if len(value) > 2:
        raise ValueError(f"data.augmentation.{block}.num_sections {value}: a number or a [min, max] pair is needed")
    if len(value) < 2:
        n = int(value[0]) if value else 0
        return n, n, False
    lo, hi = sorted(int(v) for v in value)
    return lo, hi, True


def _pick_axis(R: np.random.RandomState, axes: np.ndarray) -> int:
    return int(axes[0]) if axes.size == 1 else int(R.choice(axes))


def _pick_count(R: np.random.RandomState, count: Tuple[int, int, bool], most: int) -> int:
    lo, hi, drawn = count
    return min(max(int(R.randint(lo, hi + 1)) if drawn else lo, 0), most)


class _Block:
    """One enabled block: its settings, its RandomState and its draw."""

    def __init__(self, name: str, cfg: Dict[str, Any], seed: int):
        self.name, self.cfg = name, cfg
        self.R = np.random.RandomState((int(seed) + zlib.crc32(name.encode())) % (2 ** 32))

    def set_random_state(self, seed: Optional[int] = None, state: Optional[np.random.RandomState] = None) -> "_Block":
        self.R = state if state is not None else np.random.RandomState(seed)
        return self

    # ---- geometric: -> a signed permutation
    def draw_perm(self, dims: Sequence[int]) -> SignedPerm:
        c, R = self.cfg, self.R
        cubic = len(set(dims)) == 1
        if self.name == "axis_permute":
            if c["prob"] <= 0 or not (R.rand() < c["prob"]) or not cubic:
                return IDENTITY
            if c["include_identity"]:
                p = R.permutation(3)
            else:
                for _ in range(8):
                    p = R.permutation(3)
                    if not np.array_equal(p, np.arange(3)):
                        break
            return transpose_perm(p)
        if self.name == "rotate90_all":
            if c["prob"] <= 0 or not (R.rand() < c["prob"]) or not cubic:
                return IDENTITY
            if c["include_identity"]:
                ks = tuple(int(R.randint(0, 4)) for _ in range(3))
            else:
                for _ in range(8):
                    ks = tuple(int(R.randint(0, 4)) for _ in range(3))
                    if any(ks):
                        break
            return rotate90_all_perm(ks)
        if self.name == "flip":
            p = IDENTITY
            for ax in c["axes"]:
                if R.rand() < c["prob"]:
                    p = compose(p, flip_perm(ax))
            return p
        # rotate
        if not (R.rand() < c["prob"]):
            return IDENTITY
        return rot90_perm(int(R.randint(3)) + 1, c["axes"])

    # ---- image: -> op rows
    def draw_rows(self, dims: Sequence[int], group: int) -> List[Row]:
        c, R = self.cfg, self.R
        D, H, W = dims
        full = [0, D, 0, H, 0, W]
        name = self.name
        if name == "slice_drop":
            if c["prob"] <= 0 or c["slice_prob"] <= 0 or not (R.rand() < c["prob"]):
                return []
            axis = _pick_axis(R, c["axis_candidates"])
            cand = np.arange(dims[axis], dtype=np.int64)
            if c["preserve_boundaries"] and dims[axis] > 2:
                cand = cand[1:-1]
            if cand.size == 0:
                return []
            rows = []
            for i in cand[R.rand(cand.size) < c["slice_prob"]]:
                box = list(full)
                box[2 * axis], box[2 * axis + 1] = int(i), int(i) + 1
                rows.append(fill_row(box, float(c["fill_value"]), dims))
            return rows
        if name == "slice_shift":
            m = int(c["shift_magnitude"])
            if c["prob"] <= 0 or c["slice_prob"] <= 0 or m <= 0 or not (R.rand() < c["prob"]):
                return []
            axis = _pick_axis(R, c["axis_candidates"])
            idx = np.arange(dims[axis], dtype=np.int64)[R.rand(dims[axis]) < c["slice_prob"]]
            shifts = [(int(R.randint(-m, m + 1)), int(R.randint(-m, m + 1))) for _ in range(idx.size)]
            return [move_row(axis, int(i), int(i) + 1, du, dv, bool(c["wrap"])) for i, (du, dv) in zip(idx, shifts)]
        if name == "intensity":
            if c["banis_style"]:
                if c["mul_add_prob"] <= 0 or not (R.rand() < c["mul_add_prob"]):
                    return []
                (ml, mh), (al, ah) = sorted(float(v) for v in c["mul_range"]), sorted(float(v) for v in c["add_range"])
                mul = float(R.uniform(ml, mh))
                add = float(R.uniform(al, ah))
                return [muladd_row(mul, add)]
            if not (R.rand() < c["shift_intensity_prob"]):
                return []
            off = c["shift_intensity_offset"]
            lo, hi = (-float(off), float(off)) if np.isscalar(off) else (float(off[0]), float(off[1]))
            return [muladd_row(1.0, float(R.uniform(min(lo, hi), max(lo, hi))))]
        if name in ("slice_shift_z", "misalignment"):
            d = int(c["displacement"])
            if c["prob"] <= 0 or not (R.rand() < c["prob"]):
                return []
            R.rand()                                         # the rotation draw: rotate_ratio is 0 here, the draw is still taken
            if D <= 2:
                return []
            split = int(R.choice(np.arange(1, D - 1)))
            slip = R.rand() < 0.5
            dy0, dx0, dy1, dx1 = (int(R.randint(-d, d + 1)) for _ in range(4))
            if H <= d or W <= d:
                return []                                    # apply_misalignment_translation leaves such a volume unchanged
            if slip:
                return [move_row(0, split, split + 1, dy1, dx1, False)]
            return [move_row(0, split, D, dy1, dx1, False), move_row(0, 0, split, dy0, dx0, False)]
        if name in ("slice_drop_z", "missing_section"):
            if c["prob"] <= 0 or not (R.rand() < c["prob"]) or D <= 3:
                return []
            n = _pick_count(R, c["section_count"], D - 2)
            if n == 0:
                return []
            rows = []
            for i in R.choice(np.arange(1, D - 1), size=n, replace=False):
                value = float(R.uniform(*c["fill_value_range"]))
                if R.rand() < c["full_section_prob"]:
                    rows.append(fill_row([int(i), int(i) + 1, 0, H, 0, W], value, dims))
                    continue
                hh = max(1, int(H * R.uniform(*c["partial_ratio_range"])))
                hw = max(1, int(W * R.uniform(*c["partial_ratio_range"])))
                y0 = int(R.randint(0, max(1, H - hh + 1)))
                x0 = int(R.randint(0, max(1, W - hw + 1)))
                rows.append(fill_row([int(i), int(i) + 1, y0, y0 + hh, x0, x0 + hw], value, dims))
            return rows
        if name == "lost_section":
            if c["prob"] <= 0 or not (R.rand() < c["prob"]) or D <= 2:
                return []
            n = _pick_count(R, c["section_count"], D - 2)
            if n == 0:
                return []
            idx = R.choice(np.arange(1, D - 1), size=n, replace=False)
            dirs = R.choice(np.asarray([-1, 1], dtype=np.int64), size=n)
            mode = c["mode"]
            return [copy_row(int(i), {"previous": -1, "next": 1, "interpolate": 0}.get(mode, -1 if int(d) < 0 else 1), group)
                    for i, d in zip(idx, dirs)]
        # missing_parts
        if c["prob"] <= 0 or not (R.rand() < c["prob"]):
            return []
        ratio = R.uniform(*c["hole_range"])
        hh, hw = max(1, int(H * ratio)), max(1, int(W * ratio))
        y0 = int(R.randint(0, max(1, H - hh + 1)))
        x0 = int(R.randint(0, max(1, W - hw + 1)))
        z = int(R.randint(0, D))
        return [fill_row([z, z + 1, y0, y0 + hh, x0, x0 + hw], 0.0, dims)]


class AugmentationPlan:
    """The enabled blocks in build order, their random states, and the device call.  `.enabled` is False when there is nothing to do:
    such a plan draws nothing and launches nothing.  `.geometric`, `.image`, `.defects`: the blocks by family; `.blocks[name]`."""

    def __init__(self, aug_cfg: Any = None, *, seed: int = 0, in_channels: int = 1, do_2d: bool = False,
                 patch_size: Optional[Sequence[int]] = None):
        given = _plain(aug_cfg) if aug_cfg is not None else {}
        if not isinstance(given, dict):
            raise TypeError(f"data.augmentation must be a mapping, got {type(aug_cfg).__name__}")
        built = ", ".join(BUILT_BLOCKS)
        settings: Dict[str, Dict[str, Any]] = {}
        self.defect_mutex = False
        for key, value in given.items():
            if key in ("profile", "preset"):
                continue
            if key == "defect_mutex":
                self.defect_mutex = bool(value)
                continue
            if key in REFUSED_BLOCKS:
                if isinstance(value, dict) and bool(value.get("enabled", False)):
                    raise NotImplementedError(f"augmentation '{key}' is not built on the device (interpolating warps, blurs, noise and "
                                              f"cross-sample mixing are other work); built: {built}, defect_mutex")
                continue
            if key not in DEFAULTS:
                raise ValueError(f"unknown data.augmentation block '{key}'; known: {', '.join(sorted(DEFAULTS) + sorted(REFUSED_BLOCKS))}")
            if not isinstance(value, dict):
                raise TypeError(f"data.augmentation.{key} must be a mapping, got {type(value).__name__}")
            extra = sorted(set(value) - set(DEFAULTS[key]))
            if extra:
                raise ValueError(f"data.augmentation.{key} got unexpected keys {extra}")
            settings[key] = {**copy.deepcopy(DEFAULTS[key]), **value}
        names = [n for n in BUILT_BLOCKS if settings.get(n, {}).get("enabled", False)]
        self.seed = int(seed)
        self.blocks: Dict[str, _Block] = {}
        for name in names:
            c = settings[name]
            if name in ("slice_shift_z", "misalignment") and float(c["rotate_ratio"]) > 0:
                raise NotImplementedError(f"augmentation '{name}' with rotate_ratio {c['rotate_ratio']}: the rotation form is an "
                                          f"interpolating warp, only the translation form is built; built: {built}")
            if name == "intensity":
                if float(c["gaussian_noise_prob"]) > 0:
                    raise NotImplementedError("augmentation 'intensity' with gaussian_noise_prob > 0: device random numbers are not built; "
                                              "set it to 0 (built: banis_style mul / add, shift_intensity)")
                if not c["banis_style"] and float(c["contrast_prob"]) > 0:
                    raise NotImplementedError("augmentation 'intensity' with contrast_prob > 0: the gamma curve needs the image's min / max "
                                              "(a reduction), which is not built; set it to 0 (built: banis_style mul / add, shift_intensity)")
                if not c["banis_style"] and float(c["shift_intensity_prob"]) <= 0:
                    continue                                 # nothing of the block is left
            if name == "lost_section" and c["mode"] not in LOST_SECTION_MODES:
                raise ValueError(f"data.augmentation.lost_section.mode {c['mode']!r}: built modes are {', '.join(LOST_SECTION_MODES)}")
            if name in ("slice_drop", "slice_shift"):
                c["axis_candidates"] = _axis_candidates(name, c["spatial_axis"])
            if name in ("slice_drop_z", "missing_section", "lost_section"):
                c["section_count"] = _section_count(name, c["num_sections"])
            if name == "flip":
                ax = c["spatial_axis"]
                c["axes"] = [int(a) for a in ax] if isinstance(ax, (list, tuple)) else [int(ax)]
                if any(a < 0 or a > 2 for a in c["axes"]):
                    raise ValueError(f"flip.spatial_axis {ax}: the spatial axes of a 3-D patch are 0, 1, 2")
            if name == "rotate":
                ax = tuple(int(a) for a in (c["spatial_axes"] or (1, 2)))
                if len(ax) != 2 or ax[0] == ax[1] or any(a < 0 or a > 2 for a in ax):
                    raise ValueError(f"rotate.spatial_axes {c['spatial_axes']}: two different axes of 0, 1, 2 are needed")
                c["axes"] = ax
            self.blocks[name] = _Block(name, c, self.seed)
        self.geometric = [self.blocks[n] for n in GEOMETRIC_BLOCKS if n in self.blocks]
        self.image = [self.blocks[n] for n in IMAGE_BLOCKS if n in self.blocks]
        self.defects = [self.blocks[n] for n in DEFECT_BLOCKS if n in self.blocks]
        self.mutex_R = np.random.RandomState((self.seed + zlib.crc32(b"defect_mutex")) % (2 ** 32))
        self.enabled = bool(self.blocks)
        if self.enabled and bool(do_2d):
            raise NotImplementedError("data.augmentation with do_2d / a 2-D patch_size: only 3-D training patches are built")
        if self.enabled and int(in_channels) > 4:
            raise NotImplementedError(f"data.augmentation with in_channels {in_channels}: the reference tells a channel axis from a depth "
                                      "axis by `shape[0] <= 4`; more than 4 channels are not built")
        if patch_size is not None:
            self.check_shape(patch_size)

    @classmethod
    def from_config(cls, aug_cfg: Any, **kwargs) -> "AugmentationPlan":
        """`cfg.data.augmentation` (a mapping, a namespace or None); seed = system.seed + rank."""
        return cls(aug_cfg, **kwargs)

    def describe(self) -> str:
        return "nothing to do" if not self.enabled else ", ".join(self.blocks) + (" (defect_mutex)" if self.defect_mutex else "")

    def check_shape(self, dims: Sequence[int]) -> None:
        dims = tuple(int(v) for v in dims)
        if self.enabled and len(dims) != 3:
            raise NotImplementedError(f"data.augmentation on a {len(dims)}-D patch: only 3-D training patches are built")
        if "rotate" in self.blocks:
            a0, a1 = self.blocks["rotate"].cfg["axes"]
            if dims[a0] != dims[a1]:
                raise ValueError(f"rotate.spatial_axes {(a0, a1)} on a {dims} patch: a quarter turn of a plane with unequal sides would "
                                 "change the batch shape")

    def draw_sample(self, dims: Sequence[int]) -> Tuple[SignedPerm, List[Row]]:
        """One sample's draws in build order -> (signed permutation, image op rows)."""
        dims = tuple(int(v) for v in dims)
        perm = IDENTITY
        for b in self.geometric:
            perm = compose(perm, b.draw_perm(dims))
        rows: List[Row] = []
        for b in self.image:
            rows += b.draw_rows(dims, 0)
        if self.defect_mutex and len(self.defects) > 1:
            rows += self.defects[int(self.mutex_R.randint(len(self.defects)))].draw_rows(dims, 1)
        else:
            for g, b in enumerate(self.defects):
                rows += b.draw_rows(dims, g + 1)
        return perm, rows

    def draw_batch(self, n: int, dims: Sequence[int]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """-> perms (n, 3), ops (rows, AUG_ROW), offsets (n + 1,), all int32 and checked."""
        dims = tuple(int(v) for v in dims)
        self.check_shape(dims)
        perms = np.zeros((n, 3), dtype=np.int32)
        offsets = np.zeros(n + 1, dtype=np.int32)
        all_rows: List[Row] = []
        for i in range(n):
            perm, rows = self.draw_sample(dims)
            check_signed_perm(perm, dims)
            check_rows(rows, dims)
            perms[i] = perm
            all_rows += rows
            offsets[i + 1] = len(all_rows)
        ops = np.array(all_rows, dtype=np.int64).astype(np.int32).reshape(len(all_rows), nat.AUG_ROW)
        return perms, ops, offsets

    def __call__(self, batch: Dict[str, Any]) -> Dict[str, Any]:
        """The batch with image, label and mask (where present) augmented; tensors must lie on the device."""
        if not self.enabled:
            return batch
        image = batch["image"]
        if not isinstance(image, torch.Tensor) or not image.is_cuda:
            raise RuntimeError("image must be a CUDA(HIP) tensor: pytorch_connectomics_amd has no CPU path")
        if image.dim() != 5 or image.dtype != torch.float32:
            raise ValueError(f"image must be float32 (N, C, D, H, W), got {image.dtype} {tuple(image.shape)}")
        n, dims = int(image.shape[0]), tuple(int(v) for v in image.shape[2:])
        perms, ops, offsets = self.draw_batch(n, dims)
        return apply_tables(batch, perms, ops, offsets, checked=True)      # draw_batch has checked them


def apply_tables(batch: Dict[str, Any], perms: np.ndarray, ops: np.ndarray, offsets: np.ndarray, *,
                 checked: bool = False) -> Dict[str, Any]:
    """Upload the tables in one copy from a pinned buffer on the current stream and launch: the gather for image, label and mask, the
    defect chain for the image.  Identity permutations and empty op lists launch nothing.  Tables from outside are checked here
    (`check_signed_perm`, `check_rows`); `checked=True` says the caller has done so (the plan's own tables)."""
    from .. import hip_ops as ops_mod
    image = batch["image"]
    n = int(image.shape[0])
    dims = tuple(int(v) for v in image.shape[2:])
    perms = np.ascontiguousarray(perms, dtype=np.int32).reshape(n, 3)
    offsets = np.ascontiguousarray(offsets, dtype=np.int32).reshape(n + 1)
    ops = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1, nat.AUG_ROW)
    for i in range(0 if checked else n):
        check_signed_perm(perms[i].tolist(), dims)
        check_rows([tuple(r) for r in ops[offsets[i]:offsets[i + 1]].tolist()], dims)
    geometric = bool((perms != IDENTITY).any())
    rows = int(offsets[n])
    if not geometric and rows == 0:
        return batch
    host = torch.empty(perms.size + offsets.size + ops.size, dtype=torch.int32, pin_memory=True)
    view = host.numpy()
    view[:perms.size] = perms.ravel()
    view[perms.size:perms.size + offsets.size] = offsets
    view[perms.size + offsets.size:] = ops.ravel()
    table = host.to(image.device, non_blocking=True)
    perm_d, off_d, ops_d = table[:perms.size], table[perms.size:perms.size + offsets.size], table[perms.size + offsets.size:]
    out = dict(batch)
    if geometric:
        for key in ("image", "label", "mask"):
            t = batch.get(key)
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError(f"{key} must be a CUDA(HIP) tensor: pytorch_connectomics_amd has no CPU path")
            if t.dtype not in (torch.int32, torch.float32):
                raise TypeError(f"{key} must be int32 or float32 (4-byte elements are moved as bits), got {t.dtype}")
            if t.dim() not in (4, 5) or int(t.shape[0]) != n or tuple(int(v) for v in t.shape[-3:]) != dims:
                raise ValueError(f"{key} {tuple(t.shape)} does not match the image {tuple(image.shape)}")
            five = t.contiguous() if t.dim() == 5 else t.contiguous().unsqueeze(1)
            moved = ops_mod.augment_permute(five, perm_d, perms)
            out[key] = moved if t.dim() == 5 else moved.squeeze(1)
    if rows:
        out["image"] = ops_mod.augment_defects(out["image"].contiguous(), ops_d, off_d, ops, offsets)
    return out


def augmented_batches(batches, plan: AugmentationPlan, device):
    """Wrap a batch iterator: every tensor moves to `device`, then the plan is applied.  A plan with nothing to do is not wrapped by
    the caller (main.train_batches): the batches stay what they were."""
    for batch in batches:
        out = {k: (v.to(device, non_blocking=True) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
        yield plan(out)

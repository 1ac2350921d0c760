"""Cases of the evaluation-metric count kernel (csrc/metric_kernels.hip), shared by tests/test_host_metrics.py and
tests/test_gpu_metrics.py, and the torch reference both compare against.

A case is built on the CPU as the tensor its logits are a view of, a target and the expected counts; `logits_view(base.cuda(), ...)`
rebuilds the same layout on the GPU (a `.cuda()` of a strided view would not keep its strides).  Logits are multiples of 0.5 in [-2, 2], so equal maxima are common; the
special values a case needs (inf, NaN, -0.0, the threshold itself) are written over them at fixed places."""
from __future__ import annotations

import functools

import torch

TILE = 4096                                   # voxels per partial row (pytc_confusion_tiles); the GPU suite checks it against the library
R_SIZES = (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)
CLASSES = (1, 2, 3, 4, 5, 8, 17, 32)
LAYOUTS = ("ncdhw", "channels_last", "slice_ncdhw", "slice_channels_last")
SLICE_START, SLICE_EXTRA = 3, 5               # a slice starts at channel 3 (not 0, no multiple of 4) of a tensor 5 channels wider
VOLUME = (2, 3, 40, 36, 44)                   # 63 360 voxels per sample: 15 full tiles and a ragged one


def reference_counts(x: torch.Tensor, target: torch.Tensor, mode: str, pred_threshold: float = 0.5,
                     target_threshold: float = 0.5) -> torch.Tensor:
    """K * K + 1 int64 counts from torch ops on CPU tensors: the contract of include/pytc_hip.h pytc_confusion_counts."""
    x, target = x.detach().cpu(), target.detach().cpu()
    N, C = x.shape[:2]
    K = max(C, 2)
    x = x.reshape(N, C, -1)
    p = (x[:, 0] > pred_threshold).long() if C == 1 else torch.argmax(x, dim=1)        # CPU argmax: first maximum, NaN is the maximum
    if mode == "dense":
        t = torch.argmax(target.reshape(N, C, -1), dim=1)
        valid = torch.ones_like(t, dtype=torch.bool)
    elif mode == "threshold":
        t = (target.reshape(N, -1).to(torch.float32) > target_threshold).long()
        valid = torch.ones_like(t, dtype=torch.bool)
    else:
        raw = target.reshape(N, -1)
        raw = raw if raw.dtype.is_floating_point else raw.long()
        valid = (raw > -1) & (raw < K)
        t = torch.where(valid, raw, torch.zeros_like(raw)).long()                      # .long() truncates toward zero
    counts = torch.zeros(K * K + 1, dtype=torch.int64)
    counts[:K * K] = torch.bincount((t * K + p)[valid], minlength=K * K)
    counts[K * K] = int((~valid).sum())
    return counts


def brute_force_counts(x: torch.Tensor, target: torch.Tensor, mode: str, pred_threshold: float = 0.5,
                       target_threshold: float = 0.5) -> torch.Tensor:
    """The same table voxel by voxel in Python (small cases only): nothing shared with the torch forms."""
    import math
    N, C = x.shape[:2]
    K = max(C, 2)
    xs = x.reshape(N, C, -1).tolist()
    ts = target.reshape(N, C, -1).tolist() if mode == "dense" else target.reshape(N, -1).tolist()

    def argmax(vals):
        best, bi = vals[0], 0
        for i, v in enumerate(vals[1:], 1):
            if not math.isnan(best) and (math.isnan(v) or v > best):
                best, bi = v, i
        return bi
    counts = [0] * (K * K + 1)
    for n in range(N):
        for r in range(len(xs[n][0])):
            p = int(xs[n][0][r] > pred_threshold) if C == 1 else argmax([xs[n][c][r] for c in range(C)])
            if mode == "dense":
                t = argmax([ts[n][c][r] for c in range(C)])
            elif mode == "threshold":
                t = int(ts[n][r] > target_threshold)
            else:
                v = ts[n][r]
                t = int(v) if (isinstance(v, int) or math.isfinite(v)) and -1 < v < K else -1      # int() truncates toward zero
            counts[K * K if t < 0 else t * K + p] += 1
    return torch.tensor(counts, dtype=torch.int64)


def logits_base(N: int, C: int, shape, layout: str, seed: int) -> torch.Tensor:
    """The tensor a layout's logits are a view of: (N, C', *shape) for the NCDHW layouts, (N, *shape, C') for the channels-last ones,
    C' = C + SLICE_EXTRA for the slices.  Values: multiples of 0.5 in [-2, 2]."""
    g = torch.Generator().manual_seed(seed)
    Cw = C + SLICE_EXTRA if layout.startswith("slice") else C
    full = (N, *shape, Cw) if layout.endswith("channels_last") else (N, Cw, *shape)
    return torch.randint(-4, 5, full, generator=g).to(torch.float32) * 0.5


def logits_view(base: torch.Tensor, C: int, layout: str) -> torch.Tensor:
    """(N, C, *shape) view of `base` in `layout` (on whichever device `base` lives)."""
    if layout.endswith("channels_last"):
        base = base.permute(0, base.dim() - 1, *range(1, base.dim() - 1))
    return base[:, SLICE_START:SLICE_START + C] if layout.startswith("slice") else base


TARGET_KINDS = (("index", torch.float32), ("index", torch.int64), ("index", torch.uint8), ("threshold", torch.float32),
                ("threshold", torch.int64), ("threshold", torch.uint8), ("dense", torch.float32))


def target_kinds_for(C: int):
    return [k for k in TARGET_KINDS if (k[0] != "threshold" or C == 1) and (k[0] != "dense" or C >= 2)]


def make_target(N: int, C: int, shape, mode: str, dtype, seed: int) -> torch.Tensor:
    """Valid targets only.  index: classes in [0, K), floats with a fraction in [0, 1) added and a few -0.5 / K - 0.1 (which truncate
    to 0 and K - 1); threshold: values 0..3 (floats also 0.5, the threshold itself); dense: multiples of 0.5 with ties."""
    g = torch.Generator().manual_seed(seed + 7)
    K = max(C, 2)
    if mode == "dense":
        return torch.randint(-2, 3, (N, C, *shape), generator=g).to(torch.float32) * 0.5
    if mode == "threshold":
        t = torch.randint(0, 4, (N, 1, *shape), generator=g)
        if dtype == torch.float32:
            t = t.to(torch.float32) * 0.5                                # 0, 0.5 (not above the threshold), 1, 1.5
        return t.to(dtype)
    t = torch.randint(0, K, (N, 1, *shape), generator=g)
    if dtype == torch.float32:
        t = t.to(torch.float32) + torch.randint(0, 10, t.shape, generator=g).to(torch.float32) * 0.1
        flat = t.reshape(-1)
        flat[::7] = -0.5
        flat[3::11] = K - 0.1
        if K == 2:
            flat[5::13] = 1.9
    return t.to(dtype)


def sprinkle_specials(x: torch.Tensor, pred_threshold: float) -> None:
    """Write the special logits over a (N, C, R) view in place, at fixed voxels (where R allows)."""
    N, C, R = x.shape
    put = [float("inf"), float("-inf"), float("nan"), -0.0, pred_threshold]
    for i, v in enumerate(put):
        if 2 * i < R:
            x[0, (i * 3) % C, 2 * i] = v
    if C >= 3 and R > 12:
        x[N - 1, :3, 11] = torch.tensor([float("inf"), float("nan"), float("inf")])     # -> class 1
        x[N - 1, :, 12] = 1.25                                                          # all equal -> class 0
    if C >= 2 and R > 14:
        x[0, :, 13] = float("nan")                                                      # all NaN -> class 0
        x[0, :, 14] = float("-inf")                                                     # all -inf -> class 0


@functools.lru_cache(maxsize=None)
def sized_case(C: int, layout: str, ri: int):
    """The case of class count C, a layout and the ri-th size: N alternates 1 / 3 and the target kind cycles, so every (N, kind) pair
    appears for every C over the sizes.  -> (base, target, mode, pred_threshold, target_threshold, expected counts, N, R)."""
    R = R_SIZES[ri]
    N = 1 if (ri + CLASSES.index(C)) % 2 == 0 else 3
    kinds = target_kinds_for(C)
    mode, dtype = kinds[(ri + LAYOUTS.index(layout)) % len(kinds)]
    seed = 1000 * C + 10 * ri + LAYOUTS.index(layout)
    base = logits_base(N, C, (R,), layout, seed)
    pthr, tthr = (0.5, 0.5) if ri % 2 == 0 else (-0.5, 0.0)
    x = logits_view(base, C, layout)
    sprinkle_specials(x, pthr)
    target = make_target(N, C, (R,), mode, dtype, seed)
    if mode == "dense" and R > 3:
        target[0, 0, 3] = float("nan")
    return base, target, mode, pthr, tthr, reference_counts(x, target, mode, pthr, tthr), N, R


@functools.lru_cache(maxsize=None)
def volume_case(layout: str, C: int = VOLUME[1]):
    N, _, *shape = VOLUME
    base = logits_base(N, C, tuple(shape), layout, 77 + LAYOUTS.index(layout))
    x = logits_view(base, C, layout)
    target = make_target(N, C, tuple(shape), "index", torch.int64, 99)
    return base, target, reference_counts(x, target, "index")


def wave_cases():
    """(name, logits (1, C, 64), int64 target (1, 1, 64), the cells the 64 voxels must land in)."""
    same = torch.full((1, 32, 64), -1.0)
    same[0, 5] = 2.0
    out = [("one_cell_K32", same, torch.full((1, 1, 64), 9, dtype=torch.int64), {9 * 32 + 5: 64})]
    i = torch.arange(64)
    t, p = i % 32, (i // 32 + i) % 32
    onehot = torch.zeros(1, 32, 64)
    onehot[0, p, i] = 1.0
    assert len(set((t * 32 + p).tolist())) == 64
    out.append(("64_cells_K32", onehot, t.reshape(1, 1, 64), {int(c): 1 for c in (t * 32 + p).tolist()}))
    binary = torch.full((1, 1, 64), 3.0)
    out.append(("one_cell_K2", binary, torch.ones(1, 1, 64, dtype=torch.int64), {3: 64}))
    return out


# hand-written tables for `compute`: (name, num_classes, K x K rows, the metrics in exact fractions)
def hand_tables():
    from fractions import Fraction as Fr
    return [
        # binary: TN 50, FP 10, FN 5, TP 35
        ("binary", 1, [[50, 10], [5, 35]], {"jaccard": Fr(35, 50), "dice": Fr(70, 85), "accuracy": Fr(85, 100)}),
        ("binary_all_background", 1, [[9, 0], [0, 0]], {"jaccard": Fr(0), "dice": Fr(0), "accuracy": Fr(1)}),
        ("binary_empty", 1, [[0, 0], [0, 0]], {"jaccard": Fr(0), "dice": Fr(0), "accuracy": Fr(0)}),
        # class 2 absent from prediction and target: left out of the macro mean
        ("absent_class", 3, [[6, 2, 0], [1, 3, 0], [0, 0, 0]],
         {"jaccard": (Fr(6, 9) + Fr(3, 6)) / 2, "dice": (Fr(12, 15) + Fr(6, 9)) / 2, "accuracy": Fr(9, 12)}),
        # class 2 only predicted (never a target): present, with TP = 0
        ("only_predicted", 3, [[4, 0, 2], [0, 3, 1], [0, 0, 0]],
         {"jaccard": (Fr(4, 6) + Fr(3, 4) + Fr(0)) / 3, "dice": (Fr(8, 10) + Fr(6, 7) + Fr(0)) / 3, "accuracy": Fr(7, 10)}),
        ("multiclass_empty", 3, [[0] * 3] * 3, {"jaccard": Fr(0), "dice": Fr(0), "accuracy": Fr(0)}),
    ]

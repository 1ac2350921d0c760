"""Shared by tests/golden/make_golden_regularization.py (the REFERENCE's regularisation losses and LossOrchestrator run them) and the
regularisation tests: seeded inputs, constructor arguments, the orchestrator term lists, the shapes of the GPU suite and the
exclusion rules of its elementwise gradient check.  Everything here is plain torch on the CPU."""
import torch

LOSSES = ("BinaryRegularization", "ForegroundDistanceConsistency", "ContourDistanceConsistency", "ForegroundContourConsistency",
          "NonOverlapRegularization")
N_INPUTS = {"BinaryRegularization": 1, "ForegroundDistanceConsistency": 2, "ContourDistanceConsistency": 2,
            "ForegroundContourConsistency": 2, "NonOverlapRegularization": 1}
TAKES_MASK = {n: n != "NonOverlapRegularization" for n in LOSSES}

S1, S3, S2D = (2, 1, 4, 7, 9), (2, 3, 4, 7, 9), (2, 3, 6, 5)

# name: (loss, kwargs, shape, logit scale, mask kind)     mask kind: None | one ((N, 1, ...)) | full ((N, C, ...)); each has a zeroed slab
CASES = {
    "binary": ("BinaryRegularization", {}, S1, 1.5, None),
    "binary_mask_one": ("BinaryRegularization", {}, S3, 1.5, "one"),
    "binary_mask_full": ("BinaryRegularization", {}, S3, 1.5, "full"),
    "binary_threshold": ("BinaryRegularization", {"min_threshold": 0.05}, S1, 1.5, "full"),
    "binary_probabilities": ("BinaryRegularization", {"apply_sigmoid": False}, S1, 0.0, None),      # scale 0: inputs are uniform in (0, 1)
    "binary_wide": ("BinaryRegularization", {}, S1, 6.0, None),
    "binary_2d": ("BinaryRegularization", {}, S2D, 1.5, "one"),
    "fg_dist": ("ForegroundDistanceConsistency", {}, S1, 1.5, None),
    "fg_dist_mask_one": ("ForegroundDistanceConsistency", {}, S3, 1.5, "one"),
    "fg_dist_mask_full": ("ForegroundDistanceConsistency", {}, S3, 1.5, "full"),
    "fg_dist_wide_2d": ("ForegroundDistanceConsistency", {}, S2D, 6.0, None),
    "ct_dist": ("ContourDistanceConsistency", {}, S1, 1.5, None),
    "ct_dist_mask_one": ("ContourDistanceConsistency", {}, S3, 1.5, "one"),
    "ct_dist_mask_full": ("ContourDistanceConsistency", {}, S3, 1.5, "full"),
    "ct_dist_wide_2d": ("ContourDistanceConsistency", {}, S2D, 6.0, None),
    "fg_contour": ("ForegroundContourConsistency", {}, (2, 1, 3, 9, 11), 1.5, None),
    "fg_contour_mask": ("ForegroundContourConsistency", {}, (2, 1, 3, 9, 11), 1.5, "full"),
    "fg_contour_clamped": ("ForegroundContourConsistency", {}, (2, 1, 3, 9, 11), 6.0, "full"),
    "fg_contour_eps": ("ForegroundContourConsistency", {"eps": 1e-4}, (1, 1, 2, 5, 6), 6.0, None),
    "fg_contour_line": ("ForegroundContourConsistency", {}, (1, 1, 3, 30, 1), 1.5, None),
    "fg_contour_voxel": ("ForegroundContourConsistency", {}, (1, 1, 1, 1, 1), 1.5, None),
    "non_overlap": ("NonOverlapRegularization", {}, S3, 1.5, None),
    "non_overlap_two_channels": ("NonOverlapRegularization", {}, (2, 2, 4, 7, 9), 1.5, None),
    "non_overlap_unmasked": ("NonOverlapRegularization", {"cleft_masked": False}, S3, 1.5, None),
    "non_overlap_five_channels_2d": ("NonOverlapRegularization", {}, (2, 5, 6, 5), 6.0, None),
}


def make_tensors(loss: str, shape, scale: float, mask_kind, seed: int):
    """(inputs, mask) for one loss: `N_INPUTS[loss]` fp32 tensors of `shape` (randn x scale; uniform in (0, 1) at scale 0) and the
    mask (None, (N, 1, ...) or (N, C, ...): non-unit values, a quarter of it zero, plus a zeroed slab)."""
    g = torch.Generator().manual_seed(seed)
    inputs = [torch.rand(shape, generator=g) if scale == 0.0 else torch.randn(shape, generator=g) * scale for _ in range(N_INPUTS[loss])]
    mask = None
    if mask_kind is not None:
        mshape = tuple(shape) if mask_kind == "full" else (shape[0], 1, *shape[2:])
        mask = (torch.rand(mshape, generator=g) * 1.5 + 0.25) * (torch.rand(mshape, generator=g) > 0.25).float()
        mask[..., : max(1, shape[-1] // 4)] = 0.0
    return inputs, mask


def case_tensors(name: str):
    loss, _, shape, scale, mk = CASES[name]
    return make_tensors(loss, shape, scale, mk, 9000 + sorted(CASES).index(name))


# messages of the reference: name -> (loss, kwargs, input shapes)
ERRORS = {
    "ct_dist_shapes": ("ContourDistanceConsistency", {}, [(1, 1, 3, 4, 5), (1, 1, 3, 4, 6)]),
    "fg_contour_half_size_0": ("ForegroundContourConsistency", {"kernel_half_size": 0}, [(2, 1, 3, 6, 7), (2, 1, 3, 6, 7)]),
    "fg_contour_half_size_2": ("ForegroundContourConsistency", {"kernel_half_size": 2}, [(2, 1, 3, 6, 7), (2, 1, 3, 6, 7)]),
    "non_overlap_one_channel": ("NonOverlapRegularization", {}, [(2, 1, 3, 4, 5)]),
}

# ---- the three orchestrator runs ---------------------------------------------------------------------------------------------------
# labels: channels 0 .. 2 = targets of the three prediction channels (foreground, contour, distance), channels 3 and 4 = term masks
ORCH_TERMS = {
    # a pred_only and a pred_pred term with mask_slice, next to supervised terms, under a batch mask; logits beyond the +-20 clamp
    "plain": [
        {"function": "WeightedBCEWithLogitsLoss", "weight": 1.0, "pred_slice": "0:2", "target_slice": "0:2"},
        {"function": "WeightedMSELoss", "weight": 0.5, "pred_slice": "2:3", "target_slice": "2:3", "kwargs": {"tanh": True}},
        {"function": "BinaryRegularization", "weight": 0.01, "pred_slice": "0:1", "mask_slice": "3:4"},
        {"function": "ForegroundDistanceConsistency", "coefficient": 0.3, "pred": "0:1", "pred2": "2:3", "mask": "4:5", "call": "pred_pred"},
        {"function": "ContourDistanceConsistency", "weight": 0.2, "pred_slice": "1:2", "pred2_slice": "2:3"},
        {"function": "ForegroundContourConsistency", "weight": 0.7, "pred_slice": "0:1", "pred2_slice": "1:2", "mask_slice": "3:4"},
        {"function": "NonOverlapRegularization", "weight": 0.4, "pred_slice": "0:3", "call_kind": "pred_only"},
    ],
    # named heads: pred2 read from another head
    "heads": [
        {"function": "WeightedBCEWithLogitsLoss", "weight": 1.0, "pred_head": "mask", "target_slice": "0:2"},
        {"function": "WeightedMSELoss", "weight": 0.5, "pred_head": "sdt", "target_slice": "2:3"},
        {"function": "ForegroundDistanceConsistency", "weight": 0.3, "pred_head": "mask", "pred_slice": "0:1", "pred2_head": "sdt",
         "pred2_slice": "0:1", "mask_slice": "3:4"},
        {"function": "ContourDistanceConsistency", "weight": 0.2, "pred_head": "mask", "pred_slice": "1:2", "pred2_head": "sdt",
         "pred2_slice": "0:1"},
        {"function": "ForegroundContourConsistency", "weight": 0.7, "pred_head": "mask", "pred_slice": "0:1", "pred2_slice": "1:2"},
        {"function": "BinaryRegularization", "weight": 0.01, "pred_head": "sdt", "pred_slice": "0:1", "kwargs": {"min_threshold": 0.03}},
    ],
    # deep supervision, one regulariser kept off the deep-supervision scales
    "deep_supervision": [
        {"function": "WeightedBCEWithLogitsLoss", "weight": 1.0, "pred_slice": "0:2", "target_slice": "0:2"},
        {"function": "BinaryRegularization", "weight": 0.01, "pred_slice": "0:2", "mask_slice": "3:4"},
        {"function": "ForegroundContourConsistency", "weight": 0.7, "pred_slice": "0:1", "pred2_slice": "1:2", "mask_slice": "4:5",
         "apply_deep_supervision": False},
        {"function": "ContourDistanceConsistency", "weight": 0.2, "pred_slice": "1:2", "pred2_slice": "2:3"},
    ],
}
ORCH_HEADS = {"mask": {"out_channels": 2, "target_slice": "0:2"}, "sdt": {"out_channels": 1, "target_slice": "2:3"}}
ORCH_SHAPE = (2, 3, 4, 8, 8)
ORCH_DS_WEIGHTS = [1.0, 0.5, 0.25]


def orch_cfg(which: str):
    from types import SimpleNamespace as NS
    ds = which == "deep_supervision"
    heads = ORCH_HEADS if which == "heads" else None
    return NS(model=NS(loss=NS(deep_supervision=ds, deep_supervision_weights=ORCH_DS_WEIGHTS if ds else [1.0],
                               deep_supervision_clamp_min=-20.0, deep_supervision_clamp_max=20.0, losses=ORCH_TERMS[which],
                               loss_balancing=None, fused=True),
                       primary_head=None, heads=heads, out_channels=3),
              data=NS(label_transform=None), optimization=NS())


def orch_tensors(which: str):
    """(outputs {name: fp32 tensor}, labels (N, 5, ...), batch mask (N, 1, ...)): `output` (a dict of heads for "heads"), `ds_1`, `ds_2`
    for "deep_supervision"."""
    g = torch.Generator().manual_seed(9500 + sorted(ORCH_TERMS).index(which))
    N, _, D, H, W = ORCH_SHAPE
    outs = {}
    if which == "heads":
        outs["mask"] = torch.randn(N, 2, D, H, W, generator=g) * 9.0
        outs["sdt"] = torch.randn(N, 1, D, H, W, generator=g) * 9.0
    else:
        outs["output"] = torch.randn(ORCH_SHAPE, generator=g) * 9.0                   # beyond the +-20 clamp in places
    if which == "deep_supervision":
        outs["ds_1"] = torch.randn(N, 3, D // 2, H // 2, W // 2, generator=g) * 9.0
        outs["ds_2"] = torch.randn(N, 3, D // 4, H // 4, W // 4, generator=g) * 9.0
    labels = torch.empty(N, 5, D, H, W)
    labels[:, :2] = (torch.rand(N, 2, D, H, W, generator=g) > 0.6).float()
    labels[:, 2] = torch.rand(N, D, H, W, generator=g) * 2.0 - 1.0
    labels[:, 3:] = (torch.rand(N, 2, D, H, W, generator=g) > 0.3).float()
    mask = (torch.rand(N, 1, D, H, W, generator=g) > 0.2).float()
    return outs, labels, mask


# ---- the GPU suite: shapes, scales, masks (tests/test_gpu_regularization.py); the CPU suite checks their exclusion shares ---------------
GPU_SHAPES_1C = [(2, 1, 5, 37, 70), (1, 1, 3, 30, 4), (1, 1, 1, 5, 131), (1, 1, 2, 11, 72), (1, 1, 1, 1, 1), (1, 1, 1, 3, 3)]
GPU_SHAPE_3C = (2, 3, 5, 21, 70)
GPU_SHAPE_2D = (2, 3, 21, 9)


def gpu_cases():
    """[(id, loss, kwargs, shape, scale, mask kind)]: every single-channel shape with no mask and with an (N, 1, ...) mask, the first one
    also at scale 6; the three-channel shape with an (N, 1, ...) and an (N, C, ...) mask; the 4-D shape for the streaming kinds."""
    out = []
    for loss in LOSSES[:4]:
        for k, shape in enumerate(GPU_SHAPES_1C):
            out.append((f"{loss}-{'x'.join(map(str, shape))}-none", loss, {}, shape, 1.5, None))
            if k % 2 == 0:
                out.append((f"{loss}-{'x'.join(map(str, shape))}-one", loss, {}, shape, 1.5, "one"))
        out.append((f"{loss}-{'x'.join(map(str, GPU_SHAPES_1C[0]))}-wide", loss, {}, GPU_SHAPES_1C[0], 6.0, "full"))
        if loss != "ForegroundContourConsistency":
            for mk in ("one", "full"):
                out.append((f"{loss}-{'x'.join(map(str, GPU_SHAPE_3C))}-{mk}", loss, {}, GPU_SHAPE_3C, 1.5, mk))
            out.append((f"{loss}-{'x'.join(map(str, GPU_SHAPE_2D))}-full", loss, {}, GPU_SHAPE_2D, 1.5, "full"))
    for kw in ({}, {"cleft_masked": False}):
        tag = "masked" if not kw else "unmasked"
        out.append((f"NonOverlapRegularization-{'x'.join(map(str, GPU_SHAPE_3C))}-{tag}", "NonOverlapRegularization", kw, GPU_SHAPE_3C, 1.5, None))
    out.append((f"NonOverlapRegularization-{'x'.join(map(str, GPU_SHAPE_2D))}-wide", "NonOverlapRegularization", {}, GPU_SHAPE_2D, 6.0, None))
    out.append(("NonOverlapRegularization-2x2x1x5x131", "NonOverlapRegularization", {}, (2, 2, 1, 5, 131), 1.5, None))
    out.append(("NonOverlapRegularization-1x5x2x11x72", "NonOverlapRegularization", {}, (1, 5, 2, 11, 72), 1.5, None))
    return out


def gpu_case_tensors(case):
    cid, loss, _, shape, scale, mk = case
    return make_tensors(loss, shape, scale, mk, 9700 + [c[0] for c in gpu_cases()].index(cid))


EXCLUSION_GAP = 1e-5
EXCLUSION_CAP = 1e-3          # at most 0.1 % of a case's voxels may be flagged


def _dilate(flag: torch.Tensor, ry: int, rx: int, square: bool) -> torch.Tensor:
    """every voxel within (ry, rx) of a flagged one in its z-plane: the whole rectangle, or the cross of the two axes"""
    f = flag.float()
    H, W = f.shape[-2:]
    pad = torch.nn.functional.pad(f, (rx, rx, ry, ry))
    out = torch.zeros_like(f)
    for dy in range(-ry, ry + 1):
        for dx in range(-rx, rx + 1):
            if square or dy == 0 or dx == 0:
                out = torch.maximum(out, pad[..., ry + dy:ry + dy + H, rx + dx:rx + dx + W])
    return out > 0


def exclusions(loss: str, kwargs, inputs):
    """-> (flagged, [per-input mask of gradient elements left out of the ELEMENTWISE check]) decided in fp64 on the inputs alone.
    BinaryRegularization: voxels whose |sigmoid(x) - 0.5| lies within 1e-5 of min_threshold (the clamp's corner).
    ForegroundContourConsistency: edge voxels whose unclamped magnitude lies within 1e-5 below 1 - eps (flag a), and pooled outputs whose
    3 x 3 window has a top-two gap below 1e-5 unless both are clamped to 1 - eps (flag b).  Left out: for a the foreground voxels next
    to the edge voxel along x and y; for b the contour gradient of the output and the foreground gradient of every voxel within 2 of it
    (the window's edge voxels, and the voxels those read).  The share that is capped counts the flagged voxels."""
    x = [t.double() for t in inputs]
    none = [torch.zeros_like(t, dtype=torch.bool) for t in inputs]
    if loss == "BinaryRegularization":
        p = torch.sigmoid(x[0]) if kwargs.get("apply_sigmoid", True) else x[0]
        flag = ((p - 0.5).abs() - float(kwargs.get("min_threshold", 1e-2))).abs() < EXCLUSION_GAP
        return flag, [flag]
    if loss != "ForegroundContourConsistency":
        return none[0], none
    eps = float(kwargs.get("eps", 1e-7))
    p = torch.sigmoid(x[0])
    pp = torch.nn.functional.pad(p, (1, 1, 1, 1))
    ex = pp[..., 1:-1, :-2] - pp[..., 1:-1, 2:]
    ey = pp[..., :-2, 1:-1] - pp[..., 2:, 1:-1]
    raw = torch.sqrt(ex ** 2 + ey ** 2 + eps)
    hi = 1.0 - eps
    flag_a = (raw <= hi) & (raw > hi - EXCLUSION_GAP)
    e = raw.clamp(eps, hi)
    H, W = e.shape[-2:]
    ep = torch.nn.functional.pad(e, (1, 1, 1, 1), value=-1.0)
    win = torch.stack([ep[..., dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], -1)
    top = win.topk(2, dim=-1).values
    flag_b = ((top[..., 0] - top[..., 1]) < EXCLUSION_GAP) & ~((top[..., 0] >= hi) & (top[..., 1] >= hi)) & (top[..., 1] >= 0)
    return flag_a | flag_b, [_dilate(flag_a, 1, 1, False) | _dilate(flag_b, 2, 2, True), flag_b]

"""Seeded cases of the softmax losses, shared by tests/golden/make_golden_softmax_losses.py (which runs the reference on them),
tests/test_host_softmax_losses.py and tests/test_gpu_softmax_losses.py."""
from __future__ import annotations

import torch

# ---- CrossEntropyLossWrapper cases: name -> (kwargs, logits shape, target form) ------------------------------------------------------
# target form: "float1" = float (N, 1, ...), "long" = int64 (N, ...), "long1" = int64 (N, 1, ...)
CE_CASES = {
    "plain_3d_float1": ({}, (2, 3, 4, 6, 7), "float1"),
    "plain_3d_long": ({}, (2, 3, 4, 6, 7), "long"),
    "plain_2d_float1": ({}, (2, 4, 9, 11), "float1"),
    "plain_2d_long": ({}, (2, 4, 9, 11), "long"),
    "weight": ({"weight": [0.2, 1.0, 3.0]}, (2, 3, 4, 6, 7), "float1"),
    "ignore": ({"ignore_index": 1}, (2, 3, 4, 6, 7), "long1"),
    "ignore_default": ({}, (2, 3, 4, 6, 7), "long"),                      # some labels are -100
    "smoothing": ({"label_smoothing": 0.1}, (2, 3, 4, 6, 7), "float1"),
    "all": ({"weight": [0.2, 1.0, 3.0], "ignore_index": 2, "label_smoothing": 0.2}, (2, 3, 4, 6, 7), "long"),
    "sum": ({"reduction": "sum", "weight": [1.5, 0.5, 1.0, 2.0]}, (2, 4, 9, 11), "long1"),
    "wide_logits": ({"label_smoothing": 0.05}, (1, 5, 3, 5, 6), "float1"),
}


def ce_case_tensors(name: str):
    """-> (logits fp32, target): seeded; "ignore_default" carries -100 at a sixth of its voxels, "wide_logits" logits of sigma 15."""
    kwargs, shape, form = CE_CASES[name]
    g = torch.Generator().manual_seed(11000 + sorted(CE_CASES).index(name))
    scale = 15.0 if name == "wide_logits" else 3.0
    logits = torch.randn(shape, generator=g) * scale
    labels = torch.randint(0, shape[1], shape[:1] + shape[2:], generator=g)
    if name == "ignore_default":
        labels[torch.rand(labels.shape, generator=g) < 1.0 / 6.0] = -100
    if form == "float1":
        target = labels.unsqueeze(1).float()
    elif form == "long1":
        target = labels.unsqueeze(1)
    else:
        target = labels
    return logits, target


def ce_kwargs(name: str):
    kw = dict(CE_CASES[name][0])
    if "weight" in kw:
        kw["weight"] = torch.tensor(kw["weight"])
    return kw


# what torch refuses when the reference's wrapper is called (it checks nothing when it is constructed): name -> (kwargs, C)
CE_ERRORS = {
    "label_smoothing_above_one": ({"label_smoothing": 1.5}, 3),
    "weight_of_wrong_length": ({"weight": [1.0, 2.0]}, 3),
}

# ---- the orchestrator run: a CrossEntropyLoss term, logits beyond +-20, a batch mask, two deep-supervision scales -------------------
ORCH_TERMS = [{"function": "CrossEntropyLoss", "weight": 1.0, "target_slice": "1:2", "kwargs": {"label_smoothing": 0.1}}]
ORCH_SHAPE = (2, 3, 4, 8, 8)
ORCH_DS_WEIGHTS = [1.0, 0.5, 0.25]


def orch_cfg(ds: bool = True):
    from types import SimpleNamespace as NS
    return NS(model=NS(loss=NS(deep_supervision=ds, deep_supervision_weights=ORCH_DS_WEIGHTS if ds else [1.0],
                               deep_supervision_clamp_min=-20.0, deep_supervision_clamp_max=20.0, losses=ORCH_TERMS,
                               loss_balancing=None, fused=True),
                       primary_head=None, heads=None, out_channels=3),
              data=NS(label_transform=None), optimization=NS())


def orch_tensors():
    """(outputs {output, ds_1, ds_2}, labels (N, 2, ...): channel 0 a binary map, channel 1 the class index as float, batch mask)."""
    g = torch.Generator().manual_seed(11500)
    N, C, D, H, W = ORCH_SHAPE
    outs = {"output": torch.randn(ORCH_SHAPE, generator=g) * 12.0,
            "ds_1": torch.randn(N, C, D // 2, H // 2, W // 2, generator=g) * 12.0,
            "ds_2": torch.randn(N, C, D // 4, H // 4, W // 4, generator=g) * 12.0}
    labels = torch.empty(N, 2, D, H, W)
    labels[:, 0] = (torch.rand(N, D, H, W, generator=g) > 0.5).float()
    labels[:, 1] = torch.randint(0, C, (N, D, H, W), generator=g).float()
    mask = (torch.rand(N, 1, D, H, W, generator=g) > 0.25).float()
    return outs, labels, mask


# ---- the GPU sweep --------------------------------------------------------------------------------------------------------------------
TILE = 2048                                   # voxels per partial (pytc_softmax_loss_tiles); the GPU suite checks it against the library
GPU_SHAPES = [(2, 3, 5, 7, 9), (1, 2, 1, 5, 131), (2, 5, 3, 30, 4), (2, 4, 21, 9), (1, 32, 3, 5, 7), (2, 3, 17, 33, 65)]
LAYOUTS = ("channels_last", "contiguous", "sliced")
TARGET_KINDS = ("dense", "index_float", "index_long")
MASK_KINDS = ("none", "one", "full")


def shape_id(shape):
    return "x".join(map(str, shape))


def _seed(shape, *extra):
    s = 12000 + GPU_SHAPES.index(tuple(shape)) * 100
    for k, e in enumerate(extra):
        s += (k * 7 + 1) * e
    return s


def gpu_mask(shape, mask_kind: str):
    if mask_kind == "none":
        return None
    g = torch.Generator().manual_seed(_seed(shape, MASK_KINDS.index(mask_kind)) + 5)
    ms = (shape[0], 1 if mask_kind == "one" else shape[1]) + tuple(shape[2:])
    return (torch.rand(ms, generator=g) > 0.3).float()


def gpu_random_case(shape, target_kind: str, mask_kind: str):
    """-> (logits of sigma 4, some beyond the +-20 clamp; target; mask): dense targets are probabilities over the channel axis; index
    targets carry ignore_index = -100 at about a tenth of the voxels."""
    g = torch.Generator().manual_seed(_seed(shape, TARGET_KINDS.index(target_kind), MASK_KINDS.index(mask_kind)))
    logits = torch.randn(shape, generator=g) * 4.0
    logits.view(-1)[::97] *= 6.0
    if target_kind == "dense":
        target = torch.softmax(torch.randn(shape, generator=g) * 2.0, dim=1)
    else:
        target = torch.randint(0, shape[1], shape[:1] + tuple(shape[2:]), generator=g)
        target[torch.rand(target.shape, generator=g) < 0.1] = -100
        if target_kind == "index_float":
            target = target.float()
    return logits, target, gpu_mask(shape, mask_kind)


def gpu_exact_case(shape, target_kind: str, mask_kind: str):
    """-> (logits, target, mask, k, y): logits +20 at class k_v and -20 elsewhere, labels y_v from a second seeded map (dense: its
    one-hot form; index kinds: about a tenth of the labels are ignore_index = -100, in y too).  In fp32 the softmax is then 1 or
    exp(-40), lse is exactly 20 and -logp exactly 0 or 40."""
    g = torch.Generator().manual_seed(_seed(shape, TARGET_KINDS.index(target_kind), MASK_KINDS.index(mask_kind)) + 50)
    C = shape[1]
    sp = shape[:1] + tuple(shape[2:])
    k = torch.randint(0, C, sp, generator=g)
    y = torch.randint(0, C, sp, generator=g)
    logits = torch.full(shape, -20.0)
    logits.scatter_(1, k.unsqueeze(1), 20.0)
    if target_kind == "dense":
        target = torch.zeros(shape).scatter_(1, y.unsqueeze(1), 1.0)
    else:
        y[torch.rand(sp, generator=g) < 0.1] = -100
        target = y.float() if target_kind == "index_float" else y.clone()
    return logits, target, gpu_mask(shape, mask_kind), k, y


def to_layout(x: torch.Tensor, layout: str, device, sentinel: float = float("nan")):
    """The (N, C, *spatial) tensor on `device` in one of the three layouts -> (view, the allocation it lives in).  "sliced" = channels
    1 : 1 + C of a channels-last tensor with C + 3 channels whose other channels hold the sentinel."""
    x = x.to(device)
    if layout == "contiguous":
        out = x.contiguous()
        return out, out
    perm = (0,) + tuple(range(2, x.dim())) + (1,)            # N, *spatial, C in memory
    inv = (0, x.dim() - 1) + tuple(range(1, x.dim() - 1))
    if layout == "channels_last":
        store = x.permute(perm).contiguous()
        return store.permute(inv), store
    N, C = x.shape[:2]
    store = torch.full((N,) + tuple(x.shape[2:]) + (C + 3,), sentinel, dtype=x.dtype, device=device)
    store[..., 1:1 + C] = x.permute(perm)
    return store.permute(inv)[:, 1:1 + C], store

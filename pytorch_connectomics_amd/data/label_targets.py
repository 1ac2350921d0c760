"""`data.label_transform` on the device: an int32 instance-label patch becomes the stacked fp32 target tensor and its per-channel
`label_mask`, as the reference's MultiTaskLabelTransformd builds them on CPU workers (data/processing/transforms.py:781-950,
1027-1122; build.py:40-116), by two HIP kernels (csrc/label_target_kernels.hip): the Kisuk-Lee border erosion and one launch that
writes every channel.

    plan = LabelTargetTransform.from_config(cfg.data.label_transform)
    out = plan(label)                      # label: int32 (B, D, H, W) or (B, 1, D, H, W) on the device
    out["label"], out.get("label_mask")    # fp32 (B, C, D, H, W), bool (B, C, D, H, W); the mask only with an affinity task

Built: affinity (any offsets, deepem / banis, semantic), binary (segment_id), instance_boundary (thickness 1), polarity,
eroded_foreground.  The distance-transform, skeleton, flow, LSD and quantisation targets are refused by name.  Ids never pass through
a float: float labels are a TypeError (ids above 2^24 would merge).
"""
from __future__ import annotations

from typing import Any, Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _native as nat
from ..inference.tta_affinity import _get, _target_kwargs, _target_name, resolve_affinity_offsets_from_kwargs

# every target name the reference registers (the unknown-task message lists them)
KNOWN_TASKS = ("affinity", "binary", "decode_quantize", "energy_quantize", "eroded_foreground", "flow", "instance_boundary",
               "instance_edt", "lsd", "polarity", "sdt", "semantic_edt", "signed_distance", "skeleton_aware_edt", "small_object",
               "thin_affinity_weight")
BUILT_TASKS = ("affinity", "binary", "eroded_foreground", "instance_boundary", "polarity")
REFUSED_TASKS = tuple(n for n in KNOWN_TASKS if n not in BUILT_TASKS)
_DEFAULTS: Dict[str, Dict[str, Any]] = {
    "binary": {},
    "eroded_foreground": {"tsz_h": 2},
    "affinity": {"offsets": ["1-0-0", "0-1-0", "0-0-1"]},
    "instance_boundary": {"thickness": 1, "edge_mode": "seg-all", "mode": "3d"},
    "polarity": {"exclusive": False},
}
_ALLOWED = {
    "binary": {"segment_id"},
    "eroded_foreground": {"tsz_h"},
    "affinity": {"offsets", "long_range", "affinity_mode", "semantic"},
    "instance_boundary": {"thickness", "edge_mode", "mode"},
    "polarity": {"exclusive"},
}
RELABEL_CONNECTIVITIES = (6, 18, 26)
Half = Tuple[int, int, int]
Chain = Tuple[Half, ...]             # the erosions a source buffer went through, in order; () is the patch itself


def _plain(v: Any) -> Any:
    """config nodes (namespaces, mappings, lists) as plain Python values"""
    if isinstance(v, (str, bytes)) or v is None:
        return v
    if hasattr(v, "items"):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if hasattr(v, "__dict__") and not isinstance(v, (int, float, bool, torch.dtype)):
        return {k: _plain(x) for k, x in vars(v).items()}
    return v


def _half_size(tsz_h: Any) -> Half:
    """seg_erosion_instance's window (segment.py:48-57): a scalar erodes in-plane only, a sequence names every axis."""
    if np.isscalar(tsz_h):
        h = int(tsz_h)
        return (0, h, h)
    t = tuple(int(v) for v in tsz_h)
    if len(t) != 3:
        raise ValueError(f"tsz_h sequence length {len(t)} != seg ndim 3")
    return t


def labels_to_int32(label, what: str = "label"):
    """An integer label array or tensor as int32 with its ids intact: floats are refused (ids above 2^24 are not representable), other
    integer types are range-checked."""
    is_t = isinstance(label, torch.Tensor)
    dt = label.dtype
    floating = dt.is_floating_point if is_t else np.issubdtype(dt, np.floating)
    if floating or dt in (torch.bool, np.dtype(bool)) or (is_t and dt.is_complex):
        raise TypeError(f"{what} must hold integer instance ids, got {dt}: ids above 2^24 are not representable in float32 and would "
                        "merge")
    if dt in (torch.int32, np.dtype(np.int32)):
        return label
    if (label.numel() if is_t else label.size):
        lo, hi = (int(label.min()), int(label.max()))
        if lo < -(2 ** 31) or hi > 2 ** 31 - 1:
            raise ValueError(f"{what} ids span [{lo}, {hi}]: outside int32, which the target kernels read")
    return label.to(torch.int32) if is_t else label.astype(np.int32)


class LabelTargetTransform:
    """The planned stacked layout and the device call.  `.channels` = C, `.channel_names`, `.uses_mask`, `.sources` (the erosion chains
    the channels read), `.table` (the kernel's channel rows)."""

    def __init__(self, tasks: Sequence[Any], *, erosion: int = 0, stack_outputs: bool = True, output_dtype: Any = "float32",
                 relabel_connected_components: bool = False, relabel_connectivity: int = 6):
        # RelabelConnectedComponentsd (build.py:102-111): the pieces of an id that the crop disconnected become instances of their own,
        # before the augmentations, the erosion and the targets (`relabel`, applied by `relabelled_batches`)
        self.relabel_connected_components = bool(relabel_connected_components)
        if isinstance(relabel_connectivity, bool) or int(relabel_connectivity) != relabel_connectivity or \
                int(relabel_connectivity) not in RELABEL_CONNECTIVITIES:
            raise ValueError(f"label_transform.relabel_connectivity must be one of {RELABEL_CONNECTIVITIES}, got {relabel_connectivity!r}")
        self.relabel_connectivity = int(relabel_connectivity)
        if not bool(stack_outputs):
            raise NotImplementedError("label_transform.stack_outputs: false (one key per target) is not built: the device transform "
                                      "writes the stacked tensor")
        if output_dtype not in (None, "float32", torch.float32) and str(output_dtype).lower().strip() != "float32":
            raise NotImplementedError(f"label_transform.output_dtype {output_dtype!r}: the device transform writes float32")
        base: Chain = ()
        if int(erosion or 0) > 0:
            base = (_half_size(int(erosion)),)               # the augmentation chain erodes the patch before any target is formed
        self.global_erosion = int(erosion or 0)
        self.task_names: List[str] = []
        self.channel_names: List[str] = []
        self._rows: List[Tuple[int, Chain, int, Sequence[int]]] = []      # kind, chain, flags, v
        modes = []
        for task in tasks:
            if isinstance(task, str):
                name, kwargs = task, {}
            elif hasattr(task, "items") or hasattr(task, "__dict__"):
                name = _target_name(task)
                if name is None:
                    raise ValueError(f"Task entry {task} missing 'name'/'task'/'type'.")
                kwargs = _plain(_target_kwargs(task))
            else:
                raise TypeError(f"Unsupported task specification: {task!r}")
            if name not in KNOWN_TASKS:
                raise KeyError(f"Unknown task '{name}'. Available: {', '.join(sorted(KNOWN_TASKS))}")
            if name in REFUSED_TASKS:
                raise NotImplementedError(f"label target '{name}' is not built on the device (distance transforms, skeletons, flows, "
                                          f"LSD and quantisation are global operations); built: {', '.join(BUILT_TASKS)}")
            kw = {**_DEFAULTS[name], **kwargs}
            task_erosion = int(kw.pop("erosion", 0))
            if name == "affinity" and "affinity_mode" not in kw:
                raise ValueError("Affinity target requires kwargs.affinity_mode: 'deepem' or 'banis'.")
            extra = sorted(set(kw) - _ALLOWED[name])
            if extra:
                raise TypeError(f"label target '{name}' got unexpected kwargs {extra}")
            chain = base + ((_half_size(task_erosion),) if task_erosion > 0 else ())
            self.task_names.append(name)
            if name == "affinity":
                mode = kw["affinity_mode"]
                if mode is None:
                    raise ValueError("Affinity targets require kwargs.affinity_mode: 'deepem' or 'banis'.")
                mode_n = str(mode).strip().lower()
                if mode_n not in ("deepem", "banis"):
                    raise ValueError(f"Unsupported affinity_mode {mode!r}. Expected one of: deepem, banis.")
                modes.append(mode_n)
                offsets = resolve_affinity_offsets_from_kwargs(kw)
                semantic = bool(kw.get("semantic", False))
                if semantic:
                    non_unit = [o for o in offsets if sum(abs(v) for v in o) > 1]
                    if non_unit:
                        raise ValueError("semantic=True supports unit offsets only; got "
                                         f"{['-'.join(map(str, o)) for o in non_unit]}. Long-range affinity "
                                         "cannot be recovered from a semantic mask — two foreground voxels "
                                         "that far apart may be different objects.")
                flags = (nat.LABEL_FLAG_BANIS if mode_n == "banis" else 0) | (nat.LABEL_FLAG_SEMANTIC if semantic else 0)
                for o in offsets:
                    if any(abs(v) > 2 ** 31 - 1 for v in o):
                        raise ValueError(f"affinity offset {o} does not fit int32")
                    self._add(f"affinity[{o[0]},{o[1]},{o[2]}]", nat.LABEL_AFFINITY, chain, flags, o)
            elif name == "binary":
                ids = [int(v) for v in (kw.get("segment_id") or [])]
                if len(ids) > nat.LABEL_MAX_IDS:
                    raise NotImplementedError(f"binary with {len(ids)} segment_id entries: a channel holds at most {nat.LABEL_MAX_IDS}")
                self._add("binary", nat.LABEL_BINARY, chain, 0, ids)
            elif name == "eroded_foreground":
                self._add("eroded_foreground", nat.LABEL_BINARY, chain + (_half_size(kw["tsz_h"]),), 0, [])
            elif name == "instance_boundary":
                if int(kw["thickness"]) != 1:
                    raise NotImplementedError(f"label target 'instance_boundary' with thickness {kw['thickness']}: only thickness 1 "
                                              "(the shift-and-compare form) is built on the device")
                if kw["edge_mode"] not in nat.LABEL_EDGE_MODES:
                    raise ValueError(f"instance_boundary edge_mode must be one of {sorted(nat.LABEL_EDGE_MODES)}, got {kw['edge_mode']!r}")
                flags = nat.LABEL_EDGE_MODES[kw["edge_mode"]] | (0 if kw["mode"] == "3d" else nat.LABEL_FLAG_2D)
                self._add("instance_boundary", nat.LABEL_BOUNDARY, chain, flags, [])
            else:                                            # polarity
                if bool(kw["exclusive"]):
                    self._add("polarity", nat.LABEL_POLARITY, chain, nat.LABEL_POLARITY_EXCLUSIVE, [])
                else:
                    for part, flag in (("pos", nat.LABEL_POLARITY_POS), ("neg", nat.LABEL_POLARITY_NEG), ("fg", nat.LABEL_POLARITY_FG)):
                        self._add(f"polarity.{part}", nat.LABEL_POLARITY, chain, flag, [])
        if not self._rows:
            raise ValueError("At least one task must be specified for MultiTaskLabelTransformd.")
        if len(set(modes)) > 1:
            raise ValueError(f"Mixed affinity_mode values are not supported in one label stack: {sorted(set(modes))}")
        self.affinity_mode: Optional[str] = modes[0] if modes else None
        self.uses_mask = "affinity" in self.task_names       # only affinity makes a real per-channel mask (transforms.py:884-888)
        self.channels = len(self._rows)
        if self.channels > nat.LABEL_MAX_CHANNELS:
            raise NotImplementedError(f"{self.channels} stacked channels: one launch writes at most {nat.LABEL_MAX_CHANNELS}")
        # distinct erosion chains share one buffer each; a chain's prefixes are made first (and are buffers of their own)
        self.sources: List[Chain] = []
        for _, chain, _, _ in self._rows:
            if chain not in self.sources:
                self.sources.append(chain)
        if len(self.sources) > nat.LABEL_MAX_SOURCES:
            raise NotImplementedError(f"{len(self.sources)} distinct erosions: one launch reads at most {nat.LABEL_MAX_SOURCES} label "
                                      "buffers")
        self._steps: List[Chain] = []
        for chain in self.sources:
            for k in range(1, len(chain) + 1):
                if chain[:k] not in self._steps:
                    self._steps.append(chain[:k])
        for chain in self._steps:
            if max(chain[-1]) > nat.LABEL_MAX_EROSION:
                raise NotImplementedError(f"erosion half-size {chain[-1]}: the erosion kernel covers 0 .. {nat.LABEL_MAX_EROSION} per axis")
        self.table = (nat.LabelChannel * self.channels)()
        for row, (kind, chain, flags, v) in zip(self.table, self._rows):
            row.kind, row.source, row.flags = kind, self.sources.index(chain), flags
            row.n_ids = len(v) if kind == nat.LABEL_BINARY else 0
            for i, x in enumerate(v):
                row.v[i] = int(x)

    def _add(self, name: str, kind: int, chain: Chain, flags: int, v: Sequence[int]) -> None:
        self.channel_names.append(name)
        self._rows.append((kind, chain, flags, list(v)))

    @classmethod
    def from_config(cls, label_cfg: Any) -> "LabelTargetTransform":
        """`cfg.data.label_transform` (a mapping or a namespace): targets, erosion, stack_outputs, output_dtype,
        relabel_connected_components, relabel_connectivity."""
        targets = _get(label_cfg, "targets", None)
        if targets is None:
            targets = []
        tasks = [targets] if isinstance(targets, str) or hasattr(targets, "items") else list(targets)
        return cls(tasks, erosion=int(_get(label_cfg, "erosion", 0) or 0), stack_outputs=_get(label_cfg, "stack_outputs", True),
                   output_dtype=_get(label_cfg, "output_dtype", "float32"),
                   relabel_connected_components=bool(_get(label_cfg, "relabel_connected_components", False) or False),
                   relabel_connectivity=_none_as(_get(label_cfg, "relabel_connectivity", 6), 6))

    def describe(self) -> List[Dict[str, Any]]:
        """One plain row per channel: name, kind, source chain, flags, values (what the tests and the numpy model read)."""
        return [{"name": n, "kind": kind, "chain": chain, "flags": flags, "v": list(v)}
                for n, (kind, chain, flags, v) in zip(self.channel_names, self._rows)]

    def relabel(self, label: torch.Tensor) -> torch.Tensor:
        """The id patch with every connected piece of an id numbered on its own (hip_ops.label_cc per sample, every non-zero id a
        label, -1 among them), then -1 written back where the patch was -1 (transforms.py:573-579).  label: integer ids (B, D, H, W) or
        (B, 1, D, H, W) on the device; the shape is kept.  With the key off this is the identity: `label` itself, no launch."""
        if not self.relabel_connected_components:
            return label
        from .. import hip_ops as ops
        if not isinstance(label, torch.Tensor):
            raise TypeError(f"label must be a tensor, got {type(label).__name__}")
        ids = label[:, 0] if label.dim() == 5 and label.shape[1] == 1 else label
        if ids.dim() != 4:
            raise ValueError(f"label must be (B, D, H, W) or (B, 1, D, H, W) instance ids, got {tuple(label.shape)}")
        ids = labels_to_int32(ids)
        if not ids.is_cuda:
            raise RuntimeError("label must be a CUDA(HIP) tensor: pytorch_connectomics_amd has no CPU path")
        out, _count, _kept = ops.label_cc(ids, self.relabel_connectivity)
        out.masked_fill_(ids == -1, -1)
        return out.reshape(label.shape)

    def __call__(self, label: torch.Tensor, *, mask_dtype: torch.dtype = torch.bool) -> Dict[str, torch.Tensor]:
        from .. import hip_ops as ops
        if not isinstance(label, torch.Tensor):
            raise TypeError(f"label must be a tensor, got {type(label).__name__}")
        if label.dim() == 5 and label.shape[1] == 1:
            label = label[:, 0]
        if label.dim() != 4:
            raise ValueError(f"label must be (B, D, H, W) or (B, 1, D, H, W) instance ids, got {tuple(label.shape)}")
        label = labels_to_int32(label)
        if not label.is_cuda:
            raise RuntimeError("label must be a CUDA(HIP) tensor: pytorch_connectomics_amd has no CPU path")
        label = label.contiguous()
        made: Dict[Chain, torch.Tensor] = {(): label}
        for chain in self._steps:
            made[chain] = ops.seg_erode_instance(made[chain[:-1]], chain[-1])
        values, mask = ops.label_targets([made[c] for c in self.sources], self.table, mask=self.uses_mask, mask_dtype=mask_dtype)
        out = {"label": values}
        if mask is not None:
            out["label_mask"] = mask
        return out


def _none_as(value, default):
    return default if value is None else value


def relabelled_batches(batches: Iterable[Dict[str, torch.Tensor]], transform: LabelTargetTransform,
                       device) -> Iterator[Dict[str, torch.Tensor]]:
    """Wrap a batch iterator whose "label" holds instance ids: every tensor moves to `device` and the label goes through
    `transform.relabel`.  The seam of the reference (build.py:307-316): after the crop, before the augmentations.  The caller wraps
    nothing when the key is off."""
    for batch in batches:
        out = {k: (v.to(device, non_blocking=True) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
        out["label"] = transform.relabel(out["label"])
        yield out


def device_target_batches(batches: Iterable[Dict[str, torch.Tensor]], transform: LabelTargetTransform, device,
                          *, mask_dtype: torch.dtype = torch.float32) -> Iterator[Dict[str, torch.Tensor]]:
    """Wrap a batch iterator whose "label" holds instance ids: every tensor moves to `device`, the label becomes the stacked targets
    (and "label_mask" with an affinity task, in the form the training loop multiplies: fp32 0 / 1 by default)."""
    for batch in batches:
        out = {k: (v.to(device, non_blocking=True) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
        out.update(transform(out["label"], mask_dtype=mask_dtype))
        yield out

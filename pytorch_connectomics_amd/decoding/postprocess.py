"""`decoding.postprocessing` of a configuration on the device: the reference's apply_decoding_postprocessing (decoding/stage.py:43-124),
which runs after the decode step and before the segmentation is saved and scored.

    out = apply_decoding_postprocessing(cfg, labels)      # labels: integer ids (Z, Y, X) or (B, Z, Y, X), a device tensor or numpy

Built: `instance_cc3d: {connectivity, min_size}` -- cc3d.connected_components and cc3d.dust, here hip_ops.label_cc
(csrc/label_cc_kernels.hip) -- and `output_transpose`.  `binary` (median filter, opening, closing) is refused by name.  A device
tensor in gives a device tensor out, a numpy array in a numpy array out.

Dtypes.  After `instance_cc3d` a device tensor comes back as int32 (what the kernels write) and a numpy array as uint32: the
reference hands cc3d `spatial.astype(np.uint32)` (stage.py:101) and tests/golden/label_cc.npz records uint32 from it.  cc3d itself
picks its output dtype from the voxel count when no `out_dtype` is given; that choice could not be checked where this was written
(cc3d is not installed), so uint32 is this engine's stated choice, not a verified copy.  Without `instance_cc3d` the input's dtype
is kept."""
from __future__ import annotations

import logging
from typing import Any, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from .pipeline import _get

logger = logging.getLogger(__name__)
CONNECTIVITIES = (6, 18, 26)


class PostprocessPlan(NamedTuple):
    instance_cc3d: Optional[Tuple[int, int]]                 # (connectivity, min_size), None: not configured
    output_transpose: List[int]


def plan_postprocessing(cfg) -> Optional[PostprocessPlan]:
    """What `cfg.decoding.postprocessing` asks for, or None when it is absent or not `enabled` (stage.py:45-48).  `instance_cc3d`
    counts whenever it is not None; a node without keys gives connectivity 6 and min_size 0 (stage.py:87-93).  Refusals:
    `binary.enabled: true` (NotImplementedError), a connectivity outside 6 / 18 / 26 (ValueError: cc3d refuses it for a volume)."""
    post = _get(_get(cfg, "decoding"), "postprocessing")
    if not _get(post, "enabled", False):
        return None
    binary = _get(post, "binary")
    if binary is not None and _get(binary, "enabled", False):
        raise NotImplementedError("decoding.postprocessing.binary (median filter, opening, closing) is not built by this engine; "
                                  "instance_cc3d and output_transpose are")
    cc3d = _get(post, "instance_cc3d")
    instance = None
    if cc3d is not None:
        node = dict(cc3d.items()) if hasattr(cc3d, "items") else dict(vars(cc3d)) if hasattr(cc3d, "__dict__") else {}
        connectivity, min_size = node.get("connectivity", 6), node.get("min_size", 0)
        if isinstance(connectivity, bool) or connectivity is None or int(connectivity) != connectivity or int(connectivity) not in CONNECTIVITIES:
            raise ValueError(f"decoding.postprocessing.instance_cc3d.connectivity must be one of {CONNECTIVITIES}, got {connectivity!r}")
        if isinstance(min_size, bool) or min_size is None or int(min_size) != min_size:
            raise ValueError(f"decoding.postprocessing.instance_cc3d.min_size must be an integer, got {min_size!r}")
        instance = (int(connectivity), int(min_size))
    return PostprocessPlan(instance, [int(a) for a in (_get(post, "output_transpose") or [])])


def run_postprocessing(plan: PostprocessPlan, labels: torch.Tensor):
    """The plan on device ids -> (ids, count, kept): count / kept are the int32 device counters of hip_ops.label_cc (components
    before and after the size filter), None without `instance_cc3d`.  Nothing is read back."""
    from .. import hip_ops as ops
    out, count, kept = labels, None, None
    if plan.instance_cc3d is not None:
        connectivity, min_size = plan.instance_cc3d
        if out.dim() not in (3, 4):
            raise ValueError(f"decoding.postprocessing.instance_cc3d needs ids of shape (Z, Y, X) or (B, Z, Y, X), got {tuple(out.shape)}")
        spatial = out[0] if out.dim() == 4 else out          # stage.py:95-99: the first sample of a batch
        relabeled, count, kept = ops.label_cc(spatial, connectivity, min_size)
        out = relabeled[None] if out.dim() == 4 else relabeled
    if plan.output_transpose:
        try:
            out = out.permute(*plan.output_transpose)
        except Exception as exc:                             # stage.py:117-122: said, and the shape is kept
            logger.warning("Transpose failed with axes %s: %s. Keeping original shape.", plan.output_transpose, exc)
    return out, count, kept


def apply_decoding_postprocessing(cfg: Any, labels):
    """The reference function.  `labels` is returned as it came unless `decoding.postprocessing.enabled`."""
    plan = plan_postprocessing(cfg)
    if plan is None:
        return labels
    if isinstance(labels, torch.Tensor):
        if not labels.is_cuda:
            raise RuntimeError("labels must be a CUDA(HIP) tensor or a numpy array: pytorch_connectomics_amd has no CPU path")
        return run_postprocessing(plan, labels)[0]
    host = np.asarray(labels)
    if host.dtype.kind not in "iu":
        raise TypeError(f"labels must hold integer ids, got {host.dtype}")
    if host.dtype.kind == "u" and host.size and int(host.max()) > 2 ** 31 - 1:
        raise ValueError(f"labels ids reach {int(host.max())}: outside int32, which the component kernels read")
    dev = torch.from_numpy(np.ascontiguousarray(host.astype(np.int64) if host.dtype.itemsize > 4 or host.dtype == np.uint32 else
                                                host.astype(np.int32))).cuda()
    out = run_postprocessing(plan, dev)[0]
    return out.cpu().numpy().astype(np.uint32 if plan.instance_cc3d is not None else host.dtype, copy=False)

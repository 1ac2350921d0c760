"""decode_affinity_cc of the reference (decoding/decoders/segmentation.py:498-655) on the HIP union-find of csrc/cc_kernels.hip.

The ids are those of the reference's serial flood fill (`numba_serial`, which its `numba` and `cupy` backends reproduce) bit for bit:
background 0, components 1 .. K in raster order of their first voxel with a channel above the threshold.  A CUDA(HIP) tensor in gives the int32 device labels; a numpy array in is uploaded, decoded and returned as
the reference returns it: `fastremap.refit`, the background quirk and `cast2dtype` (`compact_labels`)."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from .registry import register_decoder

HIP_BACKENDS = ("hip", "numba", "numba_serial", "cupy", "auto")       # the reference's affinity-graph backends: one partition, one numbering


def seg_dtype(max_id: int):
    """The smallest unsigned dtype that holds max_id (data/processing/misc.py:8-17 get_seg_type; fastremap.refit picks the same)."""
    if max_id < 2 ** 8:
        return np.uint8
    if max_id < 2 ** 16:
        return np.uint16
    if max_id < 2 ** 32:
        return np.uint32
    return np.uint64


def compact_labels(labels: np.ndarray) -> np.ndarray:
    """The tail of the reference function (segmentation.py:647-655) on an integer label array: refit to the smallest unsigned dtype,
    set [0, 0, 0] to 0 when no voxel is background, cast to the dtype of the largest id that is left."""
    seg = labels.astype(seg_dtype(int(labels.max()) if labels.size else 0))
    if seg.size > 0 and not np.any(seg == 0):
        seg[(0,) * seg.ndim] = 0
    return seg.astype(seg_dtype(int(seg.max()) if seg.size else 0), copy=False)


def decode_affinity_cc(affinities, threshold: float = 0.5, backend: str = "auto", edge_offset: int = 0, orphan_fill: bool = False,
                       affinity_channels: Optional[Sequence[int]] = None):
    """Instance segmentation of affinity predictions (C, Z, Y, X), C >= 3, by connected components of the graph that joins v and
    v + unit_a where channel a > threshold at v + edge_offset unit_a (`affinity_channels`, default the first three, name the channels
    of axis 0, 1, 2).  torch.Tensor on the device -> int32 device tensor (Z, Y, X); numpy float16 / float32 array -> numpy array of the
    smallest unsigned dtype, as the reference returns it.  Refused by name: backend="cc3d" (26-connected mask components of the cc3d
    package, the reference's default, not built) and orphan_fill=True (cc3d again)."""
    import torch
    from .. import hip_ops
    if affinities.ndim != 4:
        raise ValueError(f"Expected affinities with shape (C, Z, Y, X), got {affinities.ndim}D")
    channels = (0, 1, 2)
    n_channels = int(affinities.shape[0])
    if affinity_channels is not None:
        if len(affinity_channels) != 3:
            raise ValueError(f"affinity_channels must select exactly 3 channels, got {len(affinity_channels)}")
        channels = tuple(int(c) % n_channels if -n_channels <= int(c) < n_channels else int(c) for c in affinity_channels)
        n_channels = 3
    if n_channels < 3:
        raise ValueError(f"Expected >= 3 channels, got {n_channels}")
    name = str(backend).lower()
    if name == "cc3d":
        raise NotImplementedError("backend='cc3d' (26-connected components of the foreground mask by the cc3d package) is not built: "
                                  f"the affinity-graph backends {list(HIP_BACKENDS)} run the HIP kernels")
    if name not in HIP_BACKENDS:
        raise ValueError(f"Unknown backend '{backend}'. Expected one of ['cc3d', 'numba', 'numba_serial', 'cupy', 'auto'].")
    if orphan_fill:
        raise NotImplementedError("orphan_fill=True (a second cc3d pass over the unlabeled voxels) is not built")
    if int(edge_offset) not in (0, 1):
        raise ValueError(f"edge_offset must be 0 or 1, got {edge_offset}")
    if int(np.prod(affinities.shape[1:], dtype=np.int64)) >= 2 ** 31 - 1:
        raise NotImplementedError(f"affinities of shape {tuple(affinities.shape)}: a volume of 2^31 - 1 voxels or more is not built "
                                  "(ids and indices are 31 bits)")
    if isinstance(affinities, torch.Tensor):
        labels, _count = hip_ops.affinity_cc(affinities, float(threshold), int(edge_offset), channels)
        return labels
    if not isinstance(affinities, np.ndarray) or affinities.dtype not in (np.float16, np.float32):
        raise TypeError("affinities must be a CUDA(HIP) tensor or a numpy array of float16 / float32, got "
                        f"{getattr(affinities, 'dtype', type(affinities).__name__)} (a float64 comparison is not reproduced in float32)")
    if not torch.cuda.is_available():
        raise RuntimeError("decode_affinity_cc needs an MI355X (ROCm) device: this engine has no CPU path")
    # only the three channels travel; each as its own contiguous block
    dev = torch.stack([torch.from_numpy(np.ascontiguousarray(affinities[c])) for c in channels]).cuda()
    labels, _count = hip_ops.affinity_cc(dev, float(threshold), int(edge_offset), (0, 1, 2))
    return compact_labels(labels.cpu().numpy())


register_decoder("decode_affinity_cc", decode_affinity_cc, overwrite=True)

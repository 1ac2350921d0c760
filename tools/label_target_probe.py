"""Probe of the label-target kernels (csrc/label_target_kernels.hip) on one MI355X: device-event times of the border erosion and of
the one-launch target kernel, with their algorithmic bytes and the rate that gives.

    python tools/label_target_probe.py [--iters 20] [--out profiles/label_targets_probe.txt]

Rows, each for a 4 x 112^3 batch (the MedNeXt-S training batch) and a 2 x 160^3 batch of int32 instance ids (blocky instances with
background cells and an unlabeled slab):
  erode    pytc_seg_erode_instance at half-size (0, 1, 1) (`erosion: 1`), and at (2, 2, 1) for the z-window;
           bytes = 4 (read) + 4 (write) per voxel.
  targets  pytc_label_targets for the `label_aff12` stack (12 deepem offsets, one source) with the fp32 and the uint8 mask;
           bytes = 4 sources + 4 C (+ 4 C or C for the mask) per voxel.
  batch    the whole transform call (erosion 1 + targets + fp32 mask) as the training loop makes it, by a host clock around calls
           that end in a device synchronise.
Timing: three warm-up calls, device events around one call, the median of `iters` calls (min and max beside it).  No rate is a
gate: the numbers say where the kernels stand against the streaming kernels of profiles/.
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12
AFF12 = ["0-0-1", "0-1-0", "1-0-0", "2-0-0", "3-0-0", "4-0-0", "0-0-3", "0-0-9", "0-0-27", "0-3-0", "0-9-0", "0-27-0"]


def _kernel_ms(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    return statistics.median(times), min(times), max(times)


def _call_ms(fn, iters):
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def _labels(batch, side, seed):
    """blocky instances: 14^3 cells with an id of their own, a fifth of them background, the last two x columns unlabeled"""
    rng = np.random.default_rng(seed)
    n = -(-side // 14)
    ids = rng.permutation(batch * n ** 3).reshape(batch, n, n, n).astype(np.int32) + 1
    ids[rng.random(ids.shape) < 0.2] = 0
    lab = ids.repeat(14, 1).repeat(14, 2).repeat(14, 3)[:, :side, :side, :side].copy()
    lab[..., -2:] = -1
    return torch.from_numpy(lab).cuda()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "label_targets_probe.txt"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("label_target_probe needs an MI355X: a CPU run measures nothing")
    from pytorch_connectomics_amd import hip_ops as ops
    from pytorch_connectomics_amd.data import LabelTargetTransform
    plan = LabelTargetTransform.from_config({"erosion": 1, "targets": [{"name": "affinity", "kwargs": {"offsets": AFF12,
                                                                                                       "affinity_mode": "deepem"}}]})
    C = plan.channels
    lines = [f"label_target_probe: iters {a.iters}, device {torch.cuda.get_device_name(0)}",
             "device events around one call, median (min, max) of the iterations; bytes are algorithmic: erode 4 + 4 per voxel, "
             f"targets 4 x sources + 4 C (+ 4 C fp32 mask or C uint8 mask) per voxel, C = {C}; rates against the 8 TB/s HBM peak"]

    def row(name, ms, nbytes):
        med, lo, hi = ms
        rate = nbytes / (med * 1e-3)
        lines.append(f"{name}: {med * 1e3:9.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}), {nbytes / 1e6:8.1f} MB, "
                     f"{rate / 1e12:.3f} TB/s = {100 * rate / HBM_PEAK:.1f} % of peak")

    for batch, side in ((4, 112), (2, 160)):
        label = _labels(batch, side, 9600 + side)
        vox = label.numel()
        tag = f"{batch} x {side}^3"
        out = torch.empty_like(label)
        for half in ((0, 1, 1), (2, 2, 1)):
            row(f"{tag} erode {half}      ", _kernel_ms(lambda: ops.seg_erode_instance(label, half, out=out), a.iters), vox * 8)
        eroded = ops.seg_erode_instance(label, (0, 1, 1))
        values = torch.empty((batch, C, side, side, side), dtype=torch.float32, device="cuda")
        for mask_dtype, per_voxel in ((torch.float32, 4 + 8 * C), (torch.bool, 4 + 5 * C)):
            m = torch.empty((batch, C, side, side, side), dtype=mask_dtype, device="cuda")
            row(f"{tag} targets C={C} mask {str(mask_dtype).split('.')[-1]:7s}",
                _kernel_ms(lambda: ops.label_targets([eroded], plan.table, mask_dtype=mask_dtype, values=values, mask_out=m), a.iters),
                vox * per_voxel)
            del m
        row(f"{tag} targets C={C} no mask     ",
            _kernel_ms(lambda: ops.label_targets([eroded], plan.table, mask=False, values=values), a.iters), vox * (4 + 4 * C))
        del values
        med, lo, hi = _call_ms(lambda: plan(label, mask_dtype=torch.float32), max(3, a.iters // 2))
        lines.append(f"{tag} batch : erosion 1 + targets + fp32 mask, allocations included: {med:.3f} ms per call (min {lo:.3f}, max {hi:.3f})")
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)


if __name__ == "__main__":
    main()

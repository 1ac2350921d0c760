"""Probe of the augmentation kernels (csrc/augment_kernels.hip) on one MI355X: device-event times of the signed-permutation gather and
of the image defect kernel, with their algorithmic bytes and the rate that gives.

    python tools/augment_probe.py [--iters 20] [--out profiles/augment_probe.txt]

Rows, each for a 4 x 112^3 batch (the MedNeXt-S training batch) and a 2 x 160^3 batch of one fp32 channel:
  flip     pytc_augment_permute with a flip of all three axes in every sample (no identity sample): the line kernel;
  x-moving pytc_augment_permute with z <-> x exchanged (and flipped) in every sample: the LDS tile kernel;
  copy     pytc_augment_permute with the identity in every sample, launched through the C entry (the wrapper would skip it): the
           line kernel's ceiling;
  defects  pytc_augment_defects with a 10-row chain in every sample: two multiply-adds, three fills, two shifted slabs, a lost
           section copied from its neighbour and two interpolated ones;
  no rows  pytc_augment_defects with empty op lists: the kernel's copy path;
  plan     one whole `AugmentationPlan` call on image + int32 label for tutorials/minimal_augmented.yaml's blocks (draws, one pinned
           upload, three launches), by a host clock around calls that end in a device synchronise.
Bytes are algorithmic: 4 read + 4 written per voxel and pass.  Timing: three warm-up calls, device events around one call, the median
of `iters` calls (min and max beside it).  No rate is a gate; the yardstick is the project's own streaming kernel of the same
kind, label_targets at 3.7 TB/s (profiles/label_targets_probe.txt).
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "augment_probe.txt"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("augment_probe needs an MI355X: a CPU run measures nothing")
    import ctypes as C
    from pytorch_connectomics_amd import _native as nat
    from pytorch_connectomics_amd import hip_ops as ops
    from pytorch_connectomics_amd.data import AugmentationPlan
    from pytorch_connectomics_amd.data import augment as A
    lines = [f"augment_probe: iters {a.iters}, device {torch.cuda.get_device_name(0)}",
             "device events around one call, median (min, max) of the iterations; bytes are algorithmic: 4 read + 4 written per voxel; "
             "rates against the 8 TB/s HBM peak"]

    def row(name, ms, nbytes):
        med, lo, hi = ms
        rate = nbytes / (med * 1e-3)
        lines.append(f"{name}: {med * 1e3:9.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}), {nbytes / 1e6:8.1f} MB, "
                     f"{rate / 1e12:.3f} TB/s = {100 * rate / HBM_PEAK:.1f} % of peak")

    plan_cfg = {"flip": {"enabled": True}, "rotate90_all": {"enabled": True},
                "intensity": {"enabled": True, "banis_style": True, "mul_add_prob": 1.0, "gaussian_noise_prob": 0.0},
                "missing_section": {"enabled": True, "prob": 0.5}, "misalignment": {"enabled": True, "prob": 0.5, "displacement": 8},
                "lost_section": {"enabled": True, "prob": 0.5, "num_sections": [1, 2], "mode": "interpolate"}}
    for batch, side in ((4, 112), (2, 160)):
        tag = f"{batch} x {side}^3"
        dims = (side, side, side)
        image = torch.rand((batch, 1, side, side, side), device="cuda")
        out = torch.empty_like(image)
        nbytes = image.numel() * 8
        for name, perm in (("flip    ", (-1, -2, -3)), ("x-moving", (-3, 1, 0)), ("copy    ", (0, 1, 2))):
            host = np.ascontiguousarray(np.tile(np.array(perm, dtype=np.int32), (batch, 1)))
            dev = torch.from_numpy(host.reshape(-1)).cuda()

            def launch(host=host, dev=dev):
                nat.check(nat.lib().pytc_augment_permute(C.c_void_p(image.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(dev.data_ptr()),
                                                         C.c_void_p(host.ctypes.data), batch, 1, side, side, side, ops._stream()),
                          "augment_permute")
            row(f"{tag} permute {name}", _kernel_ms(launch, a.iters), nbytes)
        chain = [A.muladd_row(1.07, 0.03), A.fill_row([5, 6, 0, side, 0, side], 0.4, dims),
                 A.fill_row([9, 10, side // 4, side // 2, side // 8, side // 2], 0.7, dims), A.move_row(0, side // 2, side, 5, -7, False),
                 A.move_row(0, 0, side // 2, -3, 4, False), A.copy_row(20, -1, 1), A.copy_row(40, 0, 1), A.copy_row(41, 0, 1),
                 A.fill_row([60, 61, 10, 30, 20, 70], 0.0, dims), A.muladd_row(0.95, -0.02)]
        A.check_rows(chain, dims)
        for name, rows_per_sample in (("10-op chain", [chain] * batch), ("no rows    ", [[]] * batch)):
            offsets = np.zeros(batch + 1, dtype=np.int32)
            offsets[1:] = np.cumsum([len(r) for r in rows_per_sample])
            flat = [r for rows in rows_per_sample for r in rows]
            table = np.array(flat, dtype=np.int64).astype(np.int32).reshape(len(flat), nat.AUG_ROW)
            table_d = torch.from_numpy(table.reshape(-1)).cuda() if len(flat) else None
            offsets_d = torch.from_numpy(offsets).cuda()
            row(f"{tag} defects {name}",
                _kernel_ms(lambda: ops.augment_defects(image, table_d, offsets_d, table if len(flat) else None, offsets, out=out), a.iters),
                nbytes)
        label = torch.randint(0, 1000, (batch, side, side, side), dtype=torch.int32, device="cuda")
        plan = AugmentationPlan(plan_cfg, seed=1)
        med, lo, hi = _call_ms(lambda: plan({"image": image, "label": label}), max(3, a.iters // 2))
        lines.append(f"{tag} plan   : {plan.describe()}; image + int32 label, draws, upload and allocations included: {med:.3f} ms per call "
                     f"(min {lo:.3f}, max {hi:.3f})")
        del image, out, label
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)


if __name__ == "__main__":
    main()

"""Probe of the id-volume connected components (csrc/label_cc_kernels.hip) on one MI355X: the time of every launch of one
`hip_ops.label_cc` call in the two forms the pipeline uses, at connectivity 6 and 26.

    python tools/label_cc_probe.py [--iters 5] [--out profiles/label_cc_probe.txt]

Every step is a child process of its own under `timeout`; the steps run one after the other and the probe stops at the first one that
fails (what ran until then is written, with the failure).  Steps:
  train:C    the relabel of a 4 x 128^3 int32 batch (`data.label_transform.relabel_connected_components`): seeded blocky ids, 24
             distinct ids on 16 x 16 x 16 blocks with a fifth of the blocks background, so an id comes back in many places.  Next to
             it the scipy model of tests/label_cc_cases.py on ONE sample and one core (scipy.ndimage.label per distinct id and the
             renumbering), and the 0.38 ms of a whole augmentation plan call (profiles/augment_probe.txt).
  decode:C   relabel plus dust (min_size 64) of a 165 x 1024 x 768 segmentation (`decoding.postprocessing.instance_cc3d`), twice: the
             ids hip_ops.affinity_cc leaves on three channels of uniform noise at threshold 0.75 (the `random` step of
             profiles/affinity_cc_probe.txt: components of every size, the parent's 4.4 .. 4.8 ms call), and blocky ids on 24^3 blocks.
Kernel times come from torch.profiler's device activities (one record per launch; median over the iterations after one warm-up call).
No number is a gate.
"""
from __future__ import annotations

import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

KERNELS = ("label_local", "label_merge", "cc_flatten", "cc_rank", "cc_scan", "cc_number", "label_bases", "label_apply", "dust_clear",
           "dust_count", "dust_kept", "dust_apply")
STEPS = [("train:6", 300), ("train:26", 300), ("decode:6", 420), ("decode:26", 420)]
AUGMENT_PLAN_MS = 0.38


def blocky_device(shape, block, n_ids, seed):
    """seeded ids 0 .. n_ids on a coarse grid, a fifth of the blocks background, upsampled on the device"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    coarse = tuple(-(-n // block) for n in shape[-3:])
    small = torch.randint(1, n_ids + 1, shape[:-3] + coarse, generator=g, device="cuda", dtype=torch.int32)
    small[torch.rand(small.shape, generator=g, device="cuda") < 0.2] = 0
    for axis in (-3, -2, -1):
        small = small.repeat_interleave(block, dim=axis)
    return small[..., :shape[-3], :shape[-2], :shape[-1]].contiguous()


def timed(fn, iters):
    import torch
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    fn()                                                     # warm-up
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    per = {}
    for ev in prof.events():
        if ev.device_type != DeviceType.CUDA:
            continue
        for name in KERNELS:
            if name + "_kernel" in ev.name:
                per.setdefault(name, []).append(float(ev.time_range.elapsed_us()))
    wall = []
    for _ in range(iters):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        t.record()
        torch.cuda.synchronize()
        wall.append(s.elapsed_time(t))
    return per, wall


def report(per, wall, voxels):
    total = 0.0
    for name in KERNELS:
        if name not in per:
            continue
        us = statistics.median(per[name])
        total += us
        print(f"  {name:12s} {us:10.1f} us (min {min(per[name]):.1f}, max {max(per[name]):.1f}, {len(per[name])} launches)")
    ms = statistics.median(wall)
    print(f"  sum of the launches {total / 1e3:.3f} ms; one call by device events {ms:.3f} ms (min {min(wall):.3f}, max {max(wall):.3f}); "
          f"{voxels / (ms * 1e-3) / 1e9:.2f} Gvoxel/s")
    return ms


def run_step(step: str, iters: int) -> None:
    import numpy as np
    import torch
    from pytorch_connectomics_amd import hip_ops
    form, connectivity = step.split(":")
    connectivity = int(connectivity)
    if form == "train":
        ids = blocky_device((4, 128, 128, 128), 16, 24, seed=1)
        _, count, _ = hip_ops.label_cc(ids, connectivity)
        print(f"{step}: relabel of {tuple(ids.shape)} int32, blocky ids: components per sample {count.tolist()}, "
              f"{100.0 * float((ids != 0).float().mean()):.1f} % foreground")
        per, wall = timed(lambda: hip_ops.label_cc(ids, connectivity), iters)
        ms = report(per, wall, ids.numel())
        print(f"  against the {AUGMENT_PLAN_MS} ms of a whole augmentation plan call (profiles/augment_probe.txt): {ms / AUGMENT_PLAN_MS:.2f} x")
        sys.path.insert(0, str(ROOT / "tests"))
        import label_cc_cases as L
        host = ids[0].cpu().numpy()
        torch.set_num_threads(1)
        t0 = time.perf_counter()
        want, k = L.model(host, connectivity)
        cpu = time.perf_counter() - t0
        same = bool(np.array_equal(want, hip_ops.label_cc(ids[0], connectivity)[0].cpu().numpy()))
        print(f"  CPU comparator: the scipy model on ONE 128^3 sample, one core: {cpu * 1e3:.0f} ms ({int(k[0])} components; equal to the "
              f"device labels: {same}); four samples {4 * cpu * 1e3:.0f} ms = {4 * cpu * 1e3 / ms:.0f} x the device call")
        return
    shape, min_size = (165, 1024, 768), 64
    g = torch.Generator(device="cuda").manual_seed(1)
    aff = torch.rand((3,) + shape, generator=g, device="cuda")
    decoded, k = hip_ops.affinity_cc(aff, 0.75, 0, (0, 1, 2))
    per_aff = []
    for _ in range(iters):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        hip_ops.affinity_cc(aff, 0.75, 0, (0, 1, 2))
        t.record()
        torch.cuda.synchronize()
        per_aff.append(s.elapsed_time(t))
    del aff
    print(f"{step}: {shape}, {decoded.numel()} voxels; hip_ops.affinity_cc on the same volume (uniform noise, threshold 0.75), "
          f"{int(k.item())} components: {statistics.median(per_aff):.3f} ms by device events")
    for kind, ids in (("decoded", decoded), ("blocky", blocky_device(shape, 24, 1000, seed=2))):
        labels, count, kept = hip_ops.label_cc(ids, connectivity, min_size)
        print(f" {kind} ids, connectivity {connectivity}, min_size {min_size}: {int(count.item())} components, {int(kept.item())} kept, "
              f"{100.0 * float((ids != 0).float().mean()):.1f} % foreground before, {100.0 * float((labels != 0).float().mean()):.1f} % after")
        del labels
        per, wall = timed(lambda: hip_ops.label_cc(ids, connectivity), iters)
        print("  relabel alone:")
        report(per, wall, ids.numel())
        per, wall = timed(lambda: hip_ops.label_cc(ids, connectivity, min_size), iters)
        print("  relabel plus dust:")
        report(per, wall, ids.numel())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "label_cc_probe.txt"))
    ap.add_argument("--step", default=None, help="run one step in this process (what the parent starts under timeout)")
    a = ap.parse_args(argv)
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("label_cc_probe needs an MI355X: a CPU run measures nothing")
        run_step(a.step, a.iters)
        return 0
    lines = [f"label_cc_probe: iters {a.iters}; kernel times from torch.profiler device activities, median over the iterations"]
    status = 0
    for step, limit in STEPS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, str(Path(__file__).resolve()), "--step", step, "--iters", str(a.iters)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        lines += [ln for ln in res.stdout.splitlines() if ln.strip()]
        print("\n".join(res.stdout.splitlines()), flush=True)
        if res.returncode != 0:
            lines.append(f"{step}: FAILED with exit status {res.returncode}; the probe stops here")
            lines += ["  " + ln for ln in res.stderr.splitlines()[-12:]]
            print(lines[-1], res.stderr[-2000:], flush=True)
            status = res.returncode
            break
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())

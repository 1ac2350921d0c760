"""Probe of the affinity connected components (csrc/cc_kernels.hip) on one MI355X: the time of every launch of one
`hip_ops.affinity_cc` call, its algorithmic bytes and the fraction of the 8 TB/s HBM peak that gives, next to the CPU a decode without
these kernels would use.

    python tools/affinity_cc_probe.py [--iters 5] [--out profiles/affinity_cc_probe.txt]

Every step is a child process of its own under `timeout`; the steps run one after the other and the probe stops at the first one that
fails (what ran until then is written, with the failure).  Steps: the shapes 112^3, 160^3 and 165 x 1024 x 768 (Lucchi++), each with
  random   three fp32 channels of uniform noise, threshold 0.75: bonds open with probability 0.25, next to the bond-percolation
           threshold of the cubic lattice (0.2488): components of every size, union chains through many tiles;
  model    the sigmoid output of tutorials/minimal_affinity_decode.yaml's untrained model on a uniform-noise volume (sliding window
           64^3, overlap 0.5), its channels (2, 1, 0) at threshold 0.5, edge_offset 1.
Kernel times come from torch.profiler's device activities (one record per launch; median over the iterations after one warm-up
call).  Algorithmic bytes per voxel: cc_edges 3 x 4 read + 1 written; cc_local 1 + 4 written; cc_merge 1 read (plus the face
voxels' parents); cc_flatten 4 read + 4 written; cc_vote 1 + 4 read; cc_rank 4 read (+ root slots); cc_number 1 read; cc_apply 4 + 4.
CPU comparator on the 112^3 and 160^3 steps: scipy.sparse.csgraph.connected_components on the same edges (one core, the graph build
included), and at every shape the device -> host copy of three fp32 channels such a decode needs first.  The reference's own numba
and cupy backends cannot run here (neither package is installed; cupy is CUDA-only), so they are not measured.  No number is a gate.
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

HBM_PEAK = 8.0e12
SHAPES = {"112": (112, 112, 112), "160": (160, 160, 160), "lucchi": (165, 1024, 768)}
STEPS = [(f"{kind}:{shape}", 240 if shape != "lucchi" else 600) for shape in SHAPES for kind in ("random", "model")]
BYTES_PER_VOXEL = {"cc_edges": 13, "cc_local": 6, "cc_merge": 1, "cc_flatten": 8, "cc_vote": 5, "cc_rank": 4, "cc_scan": 0, "cc_number": 1,
                   "cc_apply": 8}


def _affinities(kind: str, shape):
    import torch
    if kind == "random":
        g = torch.Generator(device="cuda").manual_seed(1)
        return torch.rand((3,) + tuple(shape), generator=g, device="cuda"), 0.75, 0, (0, 1, 2)
    from pytorch_connectomics_amd.config import load_config
    from pytorch_connectomics_amd.inference.window import EagerSlidingWindowEngine
    from pytorch_connectomics_amd.models import build_model
    cfg = load_config(ROOT / "tutorials" / "minimal_affinity_decode.yaml", mode="test")
    torch.manual_seed(int(cfg.system.seed))
    model = build_model(cfg).cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(2)
    vol = torch.rand((1, 1) + tuple(shape), generator=g, device="cuda")
    eng = EagerSlidingWindowEngine(roi_size=(64, 64, 64), sw_batch_size=4, overlap=0.5, mode="bump", padding_mode="constant", cval=0.0)
    with torch.no_grad():
        pred = torch.sigmoid(eng(vol, model)[0])
    return pred.contiguous(), 0.5, 1, (2, 1, 0)


def run_step(step: str, iters: int) -> None:
    import numpy as np
    import torch
    from torch.profiler import ProfilerActivity, profile
    from pytorch_connectomics_amd import hip_ops
    kind, shape_name = step.split(":")
    shape = SHAPES[shape_name]
    V = int(np.prod(shape))
    aff, thr, e, channels = _affinities(kind, shape)
    labels, count = hip_ops.affinity_cc(aff, thr, e, channels)             # warm-up
    torch.cuda.synchronize()
    K = int(count.item())
    fg = int((labels > 0).sum().item())
    sizes = torch.bincount(labels.reshape(-1))[1:]
    print(f"{step}: shape {shape}, {V} voxels, channels {channels} of {aff.shape[0]} ({aff.dtype}), threshold {thr}, edge_offset {e}: "
          f"{K} components, {100.0 * fg / V:.1f} % foreground, largest component {int(sizes.max()) if K else 0} voxels")
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            hip_ops.affinity_cc(aff, thr, e, channels)
        torch.cuda.synchronize()
    per = {}
    from torch.autograd import DeviceType
    for ev in prof.events():
        if ev.device_type != DeviceType.CUDA:
            continue
        for name in BYTES_PER_VOXEL:
            if name + "_kernel" in ev.name:
                per.setdefault(name, []).append(float(ev.time_range.elapsed_us()))
    total = 0.0
    for name in BYTES_PER_VOXEL:
        if name not in per:
            continue
        us = statistics.median(per[name])
        total += us
        nbytes = BYTES_PER_VOXEL[name] * V
        rate = nbytes / (us * 1e-6) if us > 0 else 0.0
        print(f"  {name:10s} {us:10.1f} us (min {min(per[name]):.1f}, max {max(per[name]):.1f}, {len(per[name])} launches), "
              f"{nbytes / 1e6:8.1f} MB, {rate / 1e12:.3f} TB/s = {100 * rate / HBM_PEAK:.1f} % of peak")
    wall = []
    for _ in range(iters):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        hip_ops.affinity_cc(aff, thr, e, channels)
        t.record()
        torch.cuda.synchronize()
        wall.append(s.elapsed_time(t))
    print(f"  sum of the launches {total / 1e3:.3f} ms; one call by device events {statistics.median(wall):.3f} ms "
          f"(min {min(wall):.3f}, max {max(wall):.3f}); {V / (statistics.median(wall) * 1e-3) / 1e9:.2f} Gvoxel/s")
    sel = aff[list(channels)].float().contiguous()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = sel.cpu()
    d2h = time.perf_counter() - t0
    print(f"  CPU comparator: device -> host copy of three fp32 channels ({3 * 4 * V / 1e6:.0f} MB, pageable) {d2h * 1e3:.1f} ms")
    if shape_name != "lucchi":
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        sys.path.insert(0, str(ROOT / "tests"))
        from affinity_cc_cases import edges_of
        torch.set_num_threads(1)
        t0 = time.perf_counter()
        hard = host.numpy() > np.float32(thr)
        lo, hi, _fg = edges_of(hard, e)
        n, _comp = connected_components(coo_matrix((np.ones(lo.size, dtype=np.int8), (lo, hi)), shape=(V, V)), directed=False)
        cpu = time.perf_counter() - t0
        print(f"  CPU comparator: threshold + edge list + scipy.sparse.csgraph.connected_components, one core: {cpu * 1e3:.0f} ms "
              f"({lo.size} edges; the renumbering in raster order not included)")
    else:
        print("  CPU comparator: scipy's components are not run at this size (the edge list alone is several GB)")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "affinity_cc_probe.txt"))
    ap.add_argument("--step", default=None, help="run one step in this process (what the parent starts under timeout)")
    a = ap.parse_args(argv)
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("affinity_cc_probe needs an MI355X: a CPU run measures nothing")
        run_step(a.step, a.iters)
        return 0
    lines = [f"affinity_cc_probe: iters {a.iters}; kernel times from torch.profiler device activities, median over the iterations; "
             "bytes are algorithmic (see the tool's docstring); rates against the 8 TB/s HBM peak",
             "the reference's numba and cupy backends cannot run in this image (neither package is installed; cupy is CUDA-only)"]
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

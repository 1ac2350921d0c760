"""Probe of ScnpLoss on one MI355X: loss forward + backward on the HIP kernels (csrc/scnp_kernels.hip) against the torch restatement
of the reference (ScnpLoss(use_hip=False): two gated max_pool3d passes, BCE and their autograd tape) on the same device and inputs.

    python tools/scnp_probe.py [--iters 10] [--out profiles/scnp_probe.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/scnp_probe.py --profile-only

Workload: 4 x 3 x 112^3 fp32 logits clamped to +-20 (the affinity output of the benchmark's training step), neighborhood_size 3 and
5, with a class-balancing-like C-channel weight map and without a weight.  The forward + backward figures are device events around
the whole call, median of `iters` rounds after three warm-up rounds, each round ended by a synchronise: they are end-to-end times of
the loss call and include the gaps between launches that the host-side autograd leaves, not the sum of kernel times.  Per kernel:
the median time of the launch (device events around it, in rounds of their own) and the achieved bytes per second against the
algorithmic traffic -- forward: x and t read (8 B/voxel), w read (4 B/voxel) when present, the supplier map written (1 B/voxel);
backward: x, t, w and the supplier map read, the gradient written (4 B/voxel).  --profile-only runs three HIP rounds of every row
and nothing else, for the kernel trace.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

SHAPE = (4, 3, 112, 112, 112)


def _median_ms(fn, iters: int, warmup: int = 3) -> float:
    for _ in range(warmup):
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
    return statistics.median(times)


def _inputs(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(shape, generator=g) * 6).clamp(-20, 20).cuda()
    t = (torch.rand(shape, generator=g) > 0.8).float().cuda()
    w = torch.where(t > 0, torch.full_like(t, 2.5), torch.full_like(t, 0.6))
    return x, t, w


def _step(loss, x0, t, w):
    def run():
        x = x0.detach().requires_grad_(True)
        loss(x, t, weight=w).backward()
    return run


def _kernel_rates(run, iters: int):
    """label -> (median ms, algorithmic bytes, TB/s) of the library's launches inside `run`."""
    from pytorch_connectomics_amd import hip_ops as ops
    per = {}
    for _ in range(iters):
        ops.PROFILER.records.clear()
        ops.PROFILER.enabled = True
        try:
            run()
            torch.cuda.synchronize()
        finally:
            ops.PROFILER.enabled = False
        for name, s, e, nbytes, _flops, _sym in ops.PROFILER.records:
            per.setdefault(name, ([], nbytes))[0].append(s.elapsed_time(e))
        ops.PROFILER.records.clear()
    return {k: {"ms": statistics.median(v), "bytes": b, "TB_per_s": b / (statistics.median(v) * 1e-3) / 1e12} for k, (v, b) in per.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "scnp_probe.txt"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("the probe measures on an MI355X: no device found")
    from pytorch_connectomics_amd.training.scnp_autograd import ScnpLoss
    x, t, w_full = _inputs(SHAPE)
    cases = [(ns, weighted) for ns in (3, 5) for weighted in (True, False)]
    if a.profile_only:
        for ns, weighted in cases:
            run = _step(ScnpLoss(neighborhood_size=ns), x, t, w_full if weighted else None)
            for _ in range(3):
                run()
        torch.cuda.synchronize()
        return 0
    rows = []
    for ns, weighted in cases:
        w = w_full if weighted else None
        row = {"shape": list(SHAPE), "neighborhood_size": ns, "weight": weighted}
        grads = {}
        for name, hip in (("hip", True), ("torch", False)):
            loss = ScnpLoss(neighborhood_size=ns, use_hip=hip)
            xx = x.detach().requires_grad_(True)
            v = loss(xx, t, weight=w)
            v.backward()
            row[f"{name}_loss"] = float(v.detach())
            grads[name] = xx.grad.double()
            del xx, v
            row[f"{name}_fwd_bwd_ms"] = _median_ms(_step(loss, x, t, w), a.iters)
        row["grad_rel_l2"] = float((grads["hip"] - grads["torch"]).norm() / grads["torch"].norm().clamp_min(1e-30))
        row["speedup_fwd_bwd"] = row["torch_fwd_bwd_ms"] / row["hip_fwd_bwd_ms"]
        row["kernels"] = _kernel_rates(_step(ScnpLoss(neighborhood_size=ns), x, t, w), a.iters)
        del grads
        rows.append(row)
        print(json.dumps(row), flush=True)
    text = (__doc__.strip() + "\n\n" + f"device: {torch.cuda.get_device_name()}\n\n" + json.dumps(rows, indent=1) + "\n")
    Path(a.out).write_text(text)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

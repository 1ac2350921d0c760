"""Probe of SoftClDiceLoss on one MI355X: loss forward + backward on the HIP kernels (csrc/cldice_kernels.hip) against the torch
restatement of the reference (SoftClDiceLoss(use_hip=False): max_pool3d / minimum / relu autograd) on the same device.

    python tools/soft_cldice_probe.py [--iters 10] [--out profiles/soft_cldice_probe.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/soft_cldice_probe.py --profile-only

Workloads: the `loss_soft_cldice` profile (binary, num_iters 5, sigmoid) with a class-balancing-like weight map at 4x1x112^3 and
2x1x64^3, fp32 logits clamped to +-20.  Device-event timing, median of `iters` rounds.  --profile-only runs three HIP rounds of the
112^3 case and nothing else, for the kernel trace.
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "soft_cldice_probe.txt"))
    a = ap.parse_args(argv)
    from pytorch_connectomics_amd.training.cldice_autograd import SoftClDiceLoss
    kw = {"mode": "binary", "num_iters": 5, "sigmoid": True}
    if a.profile_only:
        x, t, w = _inputs((4, 1, 112, 112, 112))
        run = _step(SoftClDiceLoss(**kw), x, t, w)
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        return 0
    rows = []
    for shape in ((4, 1, 112, 112, 112), (2, 1, 64, 64, 64)):
        x, t, w = _inputs(shape)
        row = {"shape": list(shape), "num_iters": kw["num_iters"]}
        for name, hip in (("hip", True), ("torch", False)):
            loss = SoftClDiceLoss(use_hip=hip, **kw)
            xx = x.detach().requires_grad_(True)
            v = loss(xx, t, weight=w)
            v.backward()
            row[f"{name}_loss"] = float(v)
            row[f"{name}_grad"] = xx.grad
            row[f"{name}_fwd_ms"] = _median_ms(lambda: loss(x, t, weight=w), a.iters)
            row[f"{name}_fwd_bwd_ms"] = _median_ms(_step(loss, x, t, w), a.iters)
            torch.cuda.synchronize()
            row[f"{name}_peak_mb"] = None
        gh, gt = row.pop("hip_grad").double(), row.pop("torch_grad").double()
        row["grad_rel_l2"] = float((gh - gt).norm() / gt.norm().clamp_min(1e-30))
        row["speedup_fwd_bwd"] = row["torch_fwd_bwd_ms"] / row["hip_fwd_bwd_ms"]
        for name, hip in (("hip", True), ("torch", False)):
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            _step(SoftClDiceLoss(use_hip=hip, **kw), x, t, w)()
            torch.cuda.synchronize()
            row[f"{name}_peak_mb"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        rows.append(row)
        print(json.dumps(row), flush=True)
    text = (__doc__.strip() + "\n\n" + f"device: {torch.cuda.get_device_name()}\n\n" + json.dumps(rows, indent=1) + "\n")
    Path(a.out).write_text(text)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

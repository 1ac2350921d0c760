"""Probe of the softmax losses on one MI355X: forward + backward of `CrossEntropyLoss` and of `DiceCELoss(softmax, to_onehot_y)` on
the HIP kernels (csrc/softmax_loss_kernels.hip) against the torch restatement (use_hip=False: where / log_softmax / exp / one_hot,
eight products and reductions, and their autograd tape) on the same device and inputs.

    python tools/softmax_loss_probe.py [--iters 50] [--repeats 3] [--out profiles/softmax_loss_probe.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/softmax_loss_probe.py --profile-only

Workload: 4 x C x 112^3 fp32 logits for C = 2, 3, 8, clamped to +-20, in channels-last memory (the network's output layout), a float
(N, 1, ...) class-index target, with and without a one-channel mask.  Timing: device events around `iters` forward + backward calls
after three warm-up calls; the kernels and the restatement alternate in the same process; `repeats` such measurements per row, the
median per call and the spread (min, max) over the repeats are reported.  These are end-to-end times of the loss call, host-side
autograd gaps included, not sums of kernel times.  Per kernel: the median time of its launch (device events around it, in rounds of
their own; the forward figure includes the second-stage reduction of the partials) and the achieved bytes per second against the
algorithmic traffic -- forward: 4 C + 4 label bytes per voxel (+ 4 mask bytes); backward: the same reads plus 4 C bytes of dx.
--profile-only runs three HIP rounds of every row and nothing else, for the kernel trace.
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

SPATIAL = (112, 112, 112)
CLASSES = (2, 3, 8)
LOSSES = {"CrossEntropyLoss": ("cross_entropy_loss", {}),
          "DiceCELoss": ("dice_ce_loss", {"softmax": True, "to_onehot_y": True})}


def _inputs(C, masked, seed=0):
    g = torch.Generator().manual_seed(seed + C)
    x = (torch.randn((4, C) + SPATIAL, generator=g) * 6).clamp(-20, 20).cuda().contiguous(memory_format=torch.channels_last_3d)
    y = torch.randint(0, C, (4, 1) + SPATIAL, generator=g).float().cuda()
    m = (torch.rand((4, 1) + SPATIAL, generator=g) > 0.2).float().cuda() if masked else None
    return x, y, m


def _step(fn, kw, x0, y, m, hip):
    def run():
        x = x0.detach().requires_grad_(True)
        fn(x, y, m, fill=-20.0, use_hip=hip, **kw).backward()
        return x
    return run


def _timed_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def _kernel_rates(run, iters):
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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "softmax_loss_probe.txt"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("the probe measures on an MI355X: no device found")
    from pytorch_connectomics_amd.training import softmax_loss_autograd as sl
    rows = []
    for C in CLASSES:
        for masked in (False, True):
            x, y, m = _inputs(C, masked)
            for name, (fn_name, kw) in LOSSES.items():
                fn = getattr(sl, fn_name)
                runs = {"hip": _step(fn, kw, x, y, m, True), "torch": _step(fn, kw, x, y, m, False)}
                if a.profile_only:
                    for _ in range(3):
                        runs["hip"]()
                    continue
                row = {"loss": name, "C": C, "mask": masked}
                grads = {}
                for tag, run in runs.items():
                    grads[tag] = run().grad.double()
                    row[f"{tag}_loss"] = float(fn(x, y, m, fill=-20.0, use_hip=tag == "hip", **kw))
                row["grad_rel_l2"] = float((grads["hip"] - grads["torch"]).norm() / grads["torch"].norm().clamp_min(1e-30))
                del grads
                for run in runs.values():
                    for _ in range(3):
                        run()
                torch.cuda.synchronize()
                times = {k: [] for k in runs}
                for _ in range(a.repeats):
                    for k, run in runs.items():                      # alternating in one process
                        times[k].append(_timed_ms(run, a.iters))
                for k, v in times.items():
                    row[f"{k}_fwd_bwd_ms"] = statistics.median(v)
                    row[f"{k}_fwd_bwd_ms_min_max"] = [min(v), max(v)]
                row["speedup_fwd_bwd"] = row["torch_fwd_bwd_ms"] / row["hip_fwd_bwd_ms"]
                row["kernels"] = _kernel_rates(runs["hip"], 10)
                rows.append(row)
                print(json.dumps(row), flush=True)
                del runs
                torch.cuda.empty_cache()
    torch.cuda.synchronize()
    if a.profile_only:
        return 0
    text = (__doc__.strip() + "\n\n" + f"device: {torch.cuda.get_device_name()}\n\n" + json.dumps(rows, indent=1) + "\n")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

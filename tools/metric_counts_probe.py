"""Probe of the evaluation-metric count kernel (csrc/metric_kernels.hip) on one MI355X against the paths it replaces, on the same
device and inputs, alternating in one process.

    python tools/metric_counts_probe.py [--iters 20] [--repeats 3] [--out profiles/metric_counts_probe.txt]

Rows:
  test   1 x 1 x 165 x 1024 x 768 fp32 NCDHW prediction, uint8 label (the headline volume of --mode test).
         old: what run_test did: the prediction copied to the host, then main.binary_jaccard (threshold, and, or, two sums) on the CPU;
         new: main.voxel_metrics on the device (label upload, one count call, one 5-element read).
  val    2 x 3 x 112^3 fp32 channels-last output, fp32 (N, 1, ...) class-index label (a validation batch).
         old: the torch launches validation_step ran for its Jaccard (sigmoid, two comparisons, and, or, two sums, clamp, divide);
         new: ConfusionState.update (one count call).
Timing: a host clock around calls that end in a device synchronise (the old test path ends on the host by itself); three warm-up
calls; the median of `iters` calls, and min / max over `repeats` such medians.  The kernel alone: device events around the
two launches of one pytc_confusion_counts call, median over `iters`, and its algorithmic traffic (4 C + label bytes) x voxels as
a share of the 8 TB/s HBM peak.
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

import torch  # noqa: E402

HBM_PEAK = 8.0e12


def _median_call_s(fn, iters):
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def _kernel_ms(fn, iters):
    times = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    return statistics.median(times)


def _row(name, old, new, kernel, nbytes, iters, repeats, lines):
    for fn in (old, new, kernel):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    olds, news = [], []
    for _ in range(repeats):                                # alternate the two paths
        olds.append(_median_call_s(old, iters))
        news.append(_median_call_s(new, iters))
    k_ms = _kernel_ms(kernel, iters)
    rate = nbytes / (k_ms * 1e-3)
    lines.append(f"{name}: old path {statistics.median(olds) * 1e3:9.3f} ms (min {min(olds) * 1e3:.3f}, max {max(olds) * 1e3:.3f})   "
                 f"new path {statistics.median(news) * 1e3:9.3f} ms (min {min(news) * 1e3:.3f}, max {max(news) * 1e3:.3f})")
    lines.append(f"{name}: pytc_confusion_counts (both launches) {k_ms * 1e3:9.1f} us, {nbytes / 1e6:.1f} MB algorithmic, "
                 f"{rate / 1e12:.3f} TB/s = {100 * rate / HBM_PEAK:.1f} % of the 8 TB/s HBM peak")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--test-shape", default="165,1024,768")
    ap.add_argument("--val-side", type=int, default=112)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "metric_counts_probe.txt"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("metric_counts_probe needs an MI355X: a CPU run measures nothing")
    from pytorch_connectomics_amd import hip_ops as ops
    from pytorch_connectomics_amd.main import binary_jaccard, voxel_metrics
    from pytorch_connectomics_amd.training.metrics import ConfusionState
    lines = [f"metric_counts_probe: iters {a.iters}, repeats {a.repeats}, device {torch.cuda.get_device_name(0)}",
             "old path: test = prediction to the host + binary_jaccard on the CPU; val = the torch launches of the old validation Jaccard",
             "new path: test = main.voxel_metrics on the device; val = ConfusionState.update; median call, (min, max) of the repeats' medians",
             "kernel: device events around the two launches of one pytc_confusion_counts call; bytes = (4 C + label bytes) x voxels"]
    g = torch.Generator().manual_seed(0)

    # ---- test mode -------------------------------------------------------------------------------------------------------------
    shape = tuple(int(v) for v in a.test_shape.split(","))
    pred = torch.rand((1, 1) + shape, generator=g).cuda()
    label = (torch.rand(shape, generator=g) > 0.8).to(torch.uint8)
    label_dev = label.cuda()
    old_value = binary_jaccard(pred[0, 0].float().cpu(), label)
    new_value = voxel_metrics(pred[0, 0], label)["jaccard"]
    lines.append(f"test {shape}: jaccard old {old_value!r} new {new_value!r} identical {old_value == new_value}")
    if old_value != new_value:
        raise SystemExit("\n".join(lines))
    counts = torch.zeros(5, dtype=torch.int64, device="cuda")
    vox = pred.numel()
    _row("test", lambda: binary_jaccard(pred[0, 0].float().cpu(), label), lambda: voxel_metrics(pred[0, 0], label),
         lambda: ops.confusion_counts(pred, label_dev[None, None], counts, target_mode="threshold", pred_threshold=0.5, target_threshold=0.0),
         vox * 5, max(3, a.iters // 4), a.repeats, lines)

    # ---- validation step ---------------------------------------------------------------------------------------------------------
    s = a.val_side
    out = (torch.randn((2, 3, s, s, s), generator=g) * 3).cuda().contiguous(memory_format=torch.channels_last_3d)
    lab = torch.randint(0, 3, (2, 1, s, s, s), generator=g).float().cuda()
    state = ConfusionState(3)

    def old_val():
        p = torch.sigmoid(out[:, :1].float()) > 0.5
        t = lab[:, :1] > 0
        return (p & t).sum().float() / (p | t).sum().clamp_min(1)

    counts3 = torch.zeros(10, dtype=torch.int64, device="cuda")
    _row("val ", old_val, lambda: state.update(out, lab), lambda: ops.confusion_counts(out, lab, counts3),
         out.numel() // 3 * (4 * 3 + 4), a.iters, a.repeats, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)


if __name__ == "__main__":
    main()

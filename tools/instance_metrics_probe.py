"""Probe of the label-pair table and the instance metrics (csrc/pair_table_kernels.hip) on one MI355X: the time of every launch of
one `hip_ops.label_pair_table` + `matches` call, the build's rate in algorithmic bytes against the 8 TB/s HBM peak, the scratch bytes,
the largest VOI error seen, and the CPU a score without these kernels would use.

    python tools/instance_metrics_probe.py [--iters 5] [--out profiles/instance_metrics_probe.txt]

Every step is a child process of its own under `timeout`; the steps run one after the other and the probe stops at the first one that
fails (what ran until then is written, with the failure).  Steps: `fixture` (the public functions on tests/golden/instance_metrics.npz:
the largest |VOI - the reference's recorded value| and its derived bound), then the shapes 112^3, 160^3 and 165 x 1024 x 768, each with
  decoder  the output of `hip_ops.affinity_cc` on three channels of uniform noise at threshold 0.5 (bonds open with probability 0.5,
           far above the percolation threshold: one component holds most voxels, many small ones the rest) against a blocky label of
           16 x 32 x 32 boxes;
  noise    two independent volumes of uniform ids below 2^20: nearly every voxel its own pair, P near N, U = N;
  equal    the blocky label against itself.
Kernel times come from torch.profiler's device activities (median over the iterations after one warm-up call); the whole call is
label_pair_table + record() + matches(0.5) by the host clock, the two host reads included.  Algorithmic bytes of the build: both
volumes once.  CPU comparator on the 160^3 steps, one core: the contingency table the way the reference's numpy adapted_rand and voi
build it (a scipy sparse matrix from N ones, its marginals, squares and x log2 x), after the device -> host copy of both id volumes.
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

HBM_PEAK = 8.0e12
SHAPES = {"112": (112, 112, 112), "160": (160, 160, 160), "lucchi": (165, 1024, 768)}
KINDS = ("decoder", "noise", "equal")
STEPS = [("fixture", 240)] + [(f"{kind}:{shape}", 240 if shape != "lucchi" else 600) for shape in SHAPES for kind in KINDS]
KERNELS = ("pt_runs", "pt_build", "pt_marginals", "pt_sums", "pt_finish", "pt_matches")


def _blocky(shape):
    import torch
    z, y, x = (torch.arange(n, device="cuda") for n in shape)
    ny, nx = -(-shape[1] // 32), -(-shape[2] // 32)
    ids = ((z // 16)[:, None, None] * ny + (y // 32)[None, :, None]) * nx + (x // 32)[None, None, :]
    return (ids % 7 != 0).to(torch.int32) * (ids.to(torch.int32) + 1)          # a seventh of the boxes is background


def _volumes(kind: str, shape):
    import torch
    from pytorch_connectomics_amd import hip_ops
    g = torch.Generator(device="cuda").manual_seed(3)
    if kind == "noise":
        return (torch.randint(0, 2 ** 20, shape, generator=g, device="cuda", dtype=torch.int32),
                torch.randint(0, 2 ** 20, shape, generator=g, device="cuda", dtype=torch.int32))
    label = _blocky(shape)
    if kind == "equal":
        return label.clone(), label
    seg, _count = hip_ops.affinity_cc(torch.rand((3,) + tuple(shape), generator=g, device="cuda"), 0.5, 0, (0, 1, 2))
    return seg, label


def run_fixture() -> None:
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT / "tests"))
    import instance_metric_cases as IM
    from pytorch_connectomics_amd import metrics as M
    gold = np.load(ROOT / "tests" / "golden" / "instance_metrics.npz")
    worst = (0.0, 0.0, "")
    names = sorted({k.split("__")[0] for k in gold.files})
    for name in names:
        gt, seg = gold[f"{name}__gt"], gold[f"{name}__seg"]
        rec = IM.model_record(gt, seg)
        got = M.voi(torch.from_numpy(seg).cuda(), torch.from_numpy(gt).cuda())
        for which in (0, 1):
            ref = float(gold[f"{name}__voi"][which])
            if np.isnan(ref):
                continue
            err = abs(got[which] - ref)
            if err >= worst[0]:
                worst = (err, IM.voi_tolerance(rec, ref, True, which), f"{name}[{('split', 'merge')[which]}]")
    print(f"fixture: {len(names)} label pairs; the largest |VOI - the reference's recorded float64| is {worst[0]:.3e} at {worst[2]}, "
          f"where the derived bound is {worst[1]:.3e}")


def run_step(step: str, iters: int) -> None:
    import numpy as np
    import torch
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    from pytorch_connectomics_amd import hip_ops
    from pytorch_connectomics_amd import metrics as M
    if step == "fixture":
        return run_fixture()
    kind, shape_name = step.split(":")
    shape = SHAPES[shape_name]
    V = int(np.prod(shape))
    seg, gt = _volumes(kind, shape)

    def whole():
        table = hip_ops.label_pair_table(seg, gt)
        rec = table.record()
        pairs, k = table.matches(0.5)
        return table, rec, pairs, k

    table, rec, pairs, k = whole()                                               # warm-up
    torch.cuda.synchronize()
    scratch = 48 * table.cap + 8 * 16 + 16 + 8 * max(1, rec["pairs"]) + 16
    are = M.adapted_rand_from_record(rec, True)
    split, merge = M.voi_from_record(rec)
    print(f"{step}: shape {shape}, {V} voxels, {seg.dtype} / {gt.dtype}: U {table.runs}, P {rec['pairs']}, n_true {rec['n_true']}, n_pred "
          f"{rec['n_pred']}, capacity {table.cap} slots, scratch {scratch / 1e6:.1f} MB ({scratch / V:.2f} bytes per voxel), global updates "
          f"{rec['global_updates']} from {table.workgroups} workgroups; are {float(are[0]):.6f} voi {split:.6f} / {merge:.6f}, {k} pairs at IoU >= 0.5")
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            whole()
        torch.cuda.synchronize()
    per = {}
    for ev in prof.events():
        if ev.device_type != DeviceType.CUDA:
            continue
        for name in KERNELS:
            if name + "_kernel" in ev.name:
                per.setdefault(name, []).append(float(ev.time_range.elapsed_us()))
        if "emset" in ev.name:
            per.setdefault("memset", []).append(float(ev.time_range.elapsed_us()))
    total = 0.0
    for name in KERNELS:
        if name not in per:
            continue
        us = statistics.median(per[name])
        total += us
        line = f"  {name:12s} {us:10.1f} us (min {min(per[name]):.1f}, max {max(per[name]):.1f}, {len(per[name])} launches)"
        if name in ("pt_runs", "pt_build"):
            nbytes = V * (seg.element_size() + gt.element_size())
            rate = nbytes / (us * 1e-6)
            line += f", {nbytes / 1e6:8.1f} MB, {rate / 1e12:.3f} TB/s = {100 * rate / HBM_PEAK:.1f} % of peak"
        print(line)
    if "memset" in per:
        ms = sorted(per["memset"])
        print(f"  clears       {sum(ms) / iters:10.1f} us per call in {len(ms) // iters} memsets (the tables, the record, the counters)")
        total += sum(ms) / iters
    wall = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        whole()
        wall.append((time.perf_counter() - t0) * 1e3)
    print(f"  sum of the launches and clears {total / 1e3:.3f} ms; the whole call (table, record, matches; host clock, two reads) "
          f"{statistics.median(wall):.3f} ms (min {min(wall):.3f}, max {max(wall):.3f}); {V / (statistics.median(wall) * 1e-3) / 1e9:.2f} Gvoxel/s")
    if shape_name == "112":
        sys.path.insert(0, str(ROOT / "tests"))
        import instance_metric_cases as IM
        want = IM.model_record(gt.cpu().numpy(), seg.cpu().numpy())
        exact = all(rec[c] == want[c] for c in ("N", "N1", "S_A", "S_B", "S_AB", "c", "n_true", "n_pred", "pairs"))
        errs = [abs(v - w) for v, w in zip((split, merge), want["voi"])]
        tols = [IM.voi_tolerance(want, want["voi"][i], False, i) for i in (0, 1)]
        print(f"  against the numpy model: integer cells {'equal' if exact else 'DIFFER'}; |VOI - fsum model| {errs[0]:.3e} / {errs[1]:.3e}, "
              f"derived bounds {tols[0]:.3e} / {tols[1]:.3e}")
    if shape_name == "160":
        from scipy import sparse
        torch.set_num_threads(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hs, hg = seg.cpu().numpy().ravel(), gt.cpu().numpy().ravel()
        d2h = time.perf_counter() - t0
        t0 = time.perf_counter()
        p = sparse.csr_matrix((np.ones(V, dtype=np.int64), (hg, hs)))
        rows, cols = p[1:, :], p[1:, 1:]
        a_i, b_i = np.asarray(rows.sum(1)).ravel(), np.asarray(cols.sum(0)).ravel()
        c0 = float(p[1:, 0].sum()) / V
        s_a, s_b, s_ab = float((a_i * a_i).sum()), float((b_i * b_i).sum()) + c0, float(cols.multiply(cols).sum()) + c0
        t_are = time.perf_counter() - t0
        t0 = time.perf_counter()
        w = np.ones(V)
        w[hg == 0] = 0
        cont = sparse.coo_matrix((w, (hs, hg))).tocsc()
        cont = cont / cont.sum()
        px, py = np.asarray(cont.sum(1)).ravel(), np.asarray(cont.sum(0)).ravel()
        nz = cont.data[cont.data > 0]
        h_joint = -float((nz * np.log2(nz)).sum())
        h = lambda q: -float((q[q > 0] * np.log2(q[q > 0])).sum())     # noqa: E731
        t_voi = time.perf_counter() - t0
        print(f"  CPU comparator, one core: device -> host copy of both id volumes {d2h * 1e3:.1f} ms; scipy sparse table + adapted Rand sums "
              f"{t_are * 1e3:.0f} ms (are {1 - 2 * s_ab / (s_a + s_b):.6f}); scipy contingency + entropies {t_voi * 1e3:.0f} ms "
              f"(voi {h_joint - h(py):.6f} / {h_joint - h(px):.6f})")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "instance_metrics_probe.txt"))
    ap.add_argument("--step", default=None, help="run one step in this process (what the parent starts under timeout)")
    a = ap.parse_args(argv)
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("instance_metrics_probe needs an MI355X: a CPU run measures nothing")
        run_step(a.step, a.iters)
        return 0
    lines = [f"instance_metrics_probe: iters {a.iters}; kernel times from torch.profiler device activities, median over the iterations; "
             "bytes are algorithmic (both volumes once); rates against the 8 TB/s HBM peak"]
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

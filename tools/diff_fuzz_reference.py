"""Differential fuzzing of the HOST logic of the hot path against the reference's own functions (build container only: imports
/root/reference through tests/golden/_ref_shim.py; nothing is copied).  Thousands of generated configurations / shapes per function
pair; a pair agrees when both return equal values or both raise the same exception type with the same message.

    python tools/diff_fuzz_reference.py            # prints one line per function pair + the first mismatches

Covers: sliding-window config resolvers, scan interval / patch grid, lazy window-grid builders, TTA view enumeration and ensemble
mode maps, chunk grid + halo regions, prediction crops, channel selectors."""
from __future__ import annotations

import itertools
import random
import sys
from pathlib import Path
from types import SimpleNamespace as NS

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests" / "golden"))
sys.path.insert(0, str(ROOT))
import _ref_shim as S  # noqa: E402


def outcome(fn):
    try:
        return ("ok", repr(_plain(fn())))
    except Exception as e:      # noqa: BLE001
        return ("err", type(e).__name__, str(e))


def _plain(v):
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, slice):
        return ("slice", v.start, v.stop, v.step)
    if hasattr(v, "__dataclass_fields__"):
        return {k: _plain(getattr(v, k)) for k in v.__dataclass_fields__}
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if hasattr(v, "tolist"):
        return v.tolist()
    return v


def stricter_on_purpose(name, ref, ours):
    """The two places where this package validates input the reference lets through: a chunk grid with a non-positive chunk extent
    (reference: silently EMPTY grid) and `inference.chunking.chunk_size` that is unset / too short / non-positive (reference: an
    accidental TypeError / IndexError, or a non-positive chunk shape that fails later).  Ours raises a ValueError that names the key."""
    if ours[0] != "err" or ours[1] != "ValueError":
        return False
    if name == "build_chunk_grid":
        return (ref == ("ok", "[]") or (ref[0] == "err" and ref[1] == "ZeroDivisionError")) and "must be positive" in ours[2]
    if name == "resolve_chunk_shape":
        accidental = ref[0] == "err" and (ref[1] in ("TypeError", "IndexError") or "chunk_size must be set" in ours[2])
        nonsense = ref[0] == "ok" and any(v <= 0 for v in eval(ref[1]))
        return accidental or nonsense
    return False


class Tally:
    def __init__(self):
        self.rows = []

    def run(self, name, cases, ref_fn, our_fn, show=3, same=None):
        n = bad = strict = 0
        first = []
        for case in cases:
            a, b = outcome(lambda: ref_fn(*case)), outcome(lambda: our_fn(*case))
            n += 1
            if a != b and not (same is not None and same(case, a, b)):
                if stricter_on_purpose(name, a, b):
                    strict += 1
                    continue
                bad += 1
                if len(first) < show:
                    first.append((case, a, b))
        self.rows.append((name, n, bad))
        print(f"{name:55s} cases {n:6d}  mismatches {bad}" + (f"  (+{strict} stricter on purpose)" if strict else ""))
        for case, a, b in first:
            print("    case", str(case)[:300], "\\n      ref ", str(a)[:300], "\\n      ours", str(b)[:300])


def main():
    rnd = random.Random(1234)
    t = Tally()
    rw, ow = S.ref("connectomics.inference.window"), __import__("pytorch_connectomics_amd.inference.window", fromlist=["x"])
    shapes = [tuple(rnd.randint(1, 70) for _ in range(3)) for _ in range(400)]
    rois = [tuple(rnd.randint(1, 40) for _ in range(3)) for _ in range(400)]
    overlaps = [rnd.choice([0.0, 0.25, 0.5, 0.75, 0.9, (0.25, 0.5, 0.5), (0.0, 0.5, 0.75)]) for _ in range(400)]
    t.run("compute_scan_interval", list(zip(shapes, rois, overlaps)),
          lambda s, r, o: rw.compute_scan_interval(tuple(max(a, b) for a, b in zip(s, r)), r, overlap=o),
          lambda s, r, o: ow.compute_scan_interval(tuple(max(a, b) for a, b in zip(s, r)), r, overlap=o))

    def grid(mod):
        def f(s, r, o):
            img = tuple(max(a, b) for a, b in zip(s, r))
            return mod.dense_patch_slices(img, r, mod.compute_scan_interval(img, r, overlap=o), return_slice=False)
        return f
    t.run("dense_patch_slices", list(zip(shapes[:200], rois[:200], overlaps[:200])), grid(rw), grid(ow))

    rl, ol = S.ref("connectomics.inference.lazy"), __import__("pytorch_connectomics_amd.inference.lazy", fromlist=["x"])
    ov3 = [o if isinstance(o, tuple) else (o,) * 3 for o in overlaps]
    snaps = [rnd.random() < 0.5 for _ in range(400)]
    big = [tuple(max(a, b) + rnd.randint(0, 30) for a, b in zip(s, r)) for s, r in zip(shapes, rois)]
    t.run("lazy._build_window_axis_offsets", list(zip(big, rois, ov3, snaps)),
          lambda s, r, o, sn: rl._build_window_axis_offsets(s, r, o, snap_to_edge=sn),
          lambda s, r, o, sn: ol._build_window_axis_offsets(s, r, o, snap_to_edge=sn))

    def region_case():
        for s, r, o, sn in zip(big[:250], rois[:250], ov3[:250], snaps[:250]):
            lo = tuple(rnd.randint(0, max(0, d - 1)) for d in s)
            hi = tuple(rnd.randint(l + 1, d) for l, d in zip(lo, s))
            yield s, r, o, lo, hi, sn
    t.run("lazy._build_intersecting_window_slices", list(region_case()),
          lambda s, r, o, lo, hi, sn: rl._build_intersecting_window_slices(s, r, o, region_start=lo, region_stop=hi, snap_to_edge=sn),
          lambda s, r, o, lo, hi, sn: ol._build_intersecting_window_slices(s, r, o, region_start=lo, region_stop=hi, snap_to_edge=sn))
    ctxs = [None, [], [1, 2, 2], [0, 0, 0], [40, 1, 1], [1, 2], "x", 3, [1.5, 2, 2], [-1, 0, 0]]
    t.run("lazy._resolve_target_context", [(NS(target_context=c), r) for c in ctxs for r in rois[:20]],
          rl._resolve_target_context, ol._resolve_target_context)

    rc, oc = S.ref("connectomics.inference.tta_combinations"), __import__("pytorch_connectomics_amd.inference.tta_combinations", fromlist=["x"])
    flips = [None, "all", "none", [], [[0]], [[0], [1, 2]], [0, 1], [[0, 1, 2]], [[3]], [[-1]], "z", [["a"]], [[0], [0]], [[1, 0]], 1, [[0, 0]]]
    rots = [None, [], [[1, 2]], [[0, 1], [1, 2]], "all", [[2, 1]], [[1, 1]], [[0, 3]], [1, 2], [[1, 2], [1, 2]], [["y", "x"]]]
    ks = [None, [], [1], [0, 1, 2, 3], [1, 3], [4], [5, -1], 2, ["a"]]
    combos = [(NS(flip_axes=f, rotation90_axes=r, rotate90_k=k), d) for f in flips for r in rots for k in ks for d in (2, 3)]
    t.run("resolve_tta_augmentation_combinations", combos, lambda c, d: rc.resolve_tta_augmentation_combinations(c, spatial_dims=d),
          lambda c, d: oc.resolve_tta_augmentation_combinations(c, spatial_dims=d))
    modes = ["mean", "min", "max", "median", None, [["0", "min"]], [["0:2", "min"], ["2", "max"]], [[":", "mean"]], [["5", "min"]],
             [["0", "min"], ["0", "max"]], [["0", "avg"]], [[0, "min"]], {"0": "min"}, [["0:2"]], [], "MEAN", [["1:", "max"], ["0", "min"]]]
    t.run("_resolve_ensemble_mode_map", [(m, c) for m in modes for c in (1, 2, 3, 6)], rc._resolve_ensemble_mode_map, oc._resolve_ensemble_mode_map)

    rg, og = S.ref("connectomics.chunked.chunk_grid"), __import__("pytorch_connectomics_amd.chunked.chunk_grid", fromlist=["x"])
    rh, oh = S.ref("connectomics.chunked.halo"), __import__("pytorch_connectomics_amd.chunked.halo", fromlist=["x"])
    vols = [tuple(rnd.randint(1, 90) for _ in range(3)) for _ in range(150)] + [(0, 4, 4), (4, 4), (5, 5, 5, 5)]
    chks = [tuple(rnd.randint(-1, 50) for _ in range(3)) for _ in range(150)] + [(2, 2, 2), (2, 2), (1, 1, 1)]
    t.run("build_chunk_grid", list(zip(vols, chks)), rg.build_chunk_grid, og.build_chunk_grid)

    def halo_cases():
        for v, c in zip(vols[:120], chks[:120]):
            c = tuple(max(1, x) for x in c)
            crop = tuple(rnd.randint(0, 3) for _ in range(3))
            inp = tuple(a + b + rnd.randint(0, 3) for a, b in zip(v, crop))
            halo = tuple(rnd.randint(0, 9) for _ in range(3))
            for which in (0, -1):
                yield v, c, inp, halo, crop, which
    t.run("resolve_halo_region", list(halo_cases()),
          lambda v, c, inp, h, cr, w: rh.resolve_halo_region(rg.build_chunk_grid(v, c)[w], inp, halo=h, crop_before=cr),
          lambda v, c, inp, h, cr, w: oh.resolve_halo_region(og.build_chunk_grid(v, c)[w], inp, halo=h, crop_before=cr))

    rk, ok_ = S.ref("connectomics.inference.chunk_grid"), __import__("pytorch_connectomics_amd.inference.chunk_grid", fromlist=["x"])
    pads = [None, 0, 3, [1, 2, 3], [1, 2, 3, 4, 5, 6], [[1, 2], [3, 4], [5, 6]], [1, 2], "3", [[1, 2], [3, 4]], -1, [1.5, 2, 3], [[1], [2], [3]], (2, 2, 2)]
    t.run("normalize_crop_pad", [(p,) for p in pads], rk.normalize_crop_pad, ok_.normalize_crop_pad)
    sizes = [None, [], [8, 8, 8], [100, 4, 4], [0, 4, 4], [4, 4], "8", [8, 8, 8, 8], [-1, 2, 2]]
    t.run("resolve_chunk_shape", [(NS(inference=NS(chunking=NS(chunk_size=s, axes=a))), f) for s in sizes for a in ("all", "z", "y", "ALL")
                                  for f in ((20, 30, 40), (5, 5, 5))], rk.resolve_chunk_shape, ok_.resolve_chunk_shape)
    t.run("resolve_h5_spatial_chunks", [(s,) for s in vols[:60]], rk.resolve_h5_spatial_chunks, ok_.resolve_h5_spatial_chunks)

    rs, os_ = S.ref("connectomics.utils.channel_slices"), __import__("pytorch_connectomics_amd.utils.channel_slices", fromlist=["x"])
    sels = [None, 0, 3, -1, -9, True, "2", " -2 ", ":", "1:", ":3", "1:3", "-3:-1", ":-2", "5:2", "0:0", "1:2:3", "a:b", "", "x", [0, 2], [3, -5, "1"],
            [], [0.5], 1.5, (1, 4), "7", "-7:", [0, 0], ["a"], "1 : 3", "+1", b"1"]
    for fn in ("normalize_channel_selector", "normalize_channel_range_selector", "infer_min_required_channels"):
        t.run(f"channel_slices.{fn}", [(s,) for s in sels], lambda s, fn=fn: getattr(rs, fn)(s, context="c"), lambda s, fn=fn: getattr(os_, fn)(s, context="c"))
    for fn in ("resolve_channel_indices", "resolve_channel_range"):
        t.run(f"channel_slices.{fn}", [(s, n) for s in sels for n in (0, 1, 3, 7)],
              lambda s, n, fn=fn: getattr(rs, fn)(s, num_channels=n, context="c"), lambda s, n, fn=fn: getattr(os_, fn)(s, num_channels=n, context="c"))
    affinity_views(t, rnd)
    prediction_crops(t, rnd)
    blending_maps(t, rnd)
    output_transforms(t, rnd)
    training_host_side(t, rnd)
    predictor_orchestration(t, rnd)
    model_builders(t, rnd)
    lazy_accessor_geometry(t, rnd)
    lazy_engine(t, rnd)
    chunked_runner(t, rnd)
    loss_orchestration(t, rnd)
    output_files(t, rnd)
    eager_engine(t, rnd)
    small_resolvers(t, rnd)
    patch_first_local(t, rnd)
    total, bad = sum(r[1] for r in t.rows), sum(r[2] for r in t.rows)
    print(f"TOTAL {total} cases, {bad} mismatches over {len(t.rows)} function pairs")
    return bad


def affinity_views(t, rnd):
    """Affinity-aware TTA end to end: plan construction (or its refusal) and, per view, the inverted prediction + the validity of
    every channel -- reference `build_affinity_tta_plan` + `invert_view` against this package's."""
    import torch
    ra, oa = S.ref("connectomics.inference.tta_affinity"), __import__("pytorch_connectomics_amd.inference.tta_affinity", fromlist=["x"])
    rc, oc = S.ref("connectomics.inference.tta_combinations"), __import__("pytorch_connectomics_amd.inference.tta_combinations", fromlist=["x"])
    unit = ["1-0-0", "0-1-0", "0-0-1"]
    offset_sets = [unit, unit + ["3-0-0", "0-3-0", "0-0-3"], unit + ["2-0-0", "0-4-0", "0-0-4"], ["0-1-0", "0-0-1"], ["1-0-0"],
                   unit + ["1-1-0"], ["0-1-1", "0-1--1"], unit + ["0-9-0", "0-0-9"], ["1-0-0", "0-1-0", "0-0-1", "1-0-0"]]
    tta_sets = [dict(flip_axes="all", rotation90_axes=None), dict(flip_axes=[[0]], rotation90_axes=[[1, 2]]),
                dict(flip_axes="all", rotation90_axes=[[1, 2]]), dict(flip_axes=[[1], [2]], rotation90_axes=None),
                dict(flip_axes=None, rotation90_axes=[[1, 2]], rotate90_k=[1, 3]), dict(flip_axes=[[0, 1, 2]], rotation90_axes=[[0, 1]])]
    cases = []
    for offs in offset_sets:
        for mode in ("deepem", "banis"):
            for tk in tta_sets:
                for extra_before, extra_after in ((0, 0), (1, 0), (0, 2)):
                    targets = [{"name": "binary"}] * extra_before + [{"name": "affinity", "kwargs": {"offsets": offs, "affinity_mode": mode}}] \
                        + [{"name": "binary"}] * extra_after
                    width = extra_before + len(offs) + extra_after
                    heads, req = None, None
                    if rnd.random() < 0.3:
                        heads, req = {"aff": {"out_channels": len(offs), "target_slice": f"{extra_before}:{extra_before + len(offs)}"},
                                      "aux": {"out_channels": 1}}, "aff"
                    cases.append((targets, width if heads is None else len(offs), heads, req, tk))

    def run(mod_a, mod_c, targets, num_raw, heads, req, tk):
        cfg = NS(model=NS(primary_head=None, heads=heads, out_channels=num_raw),
                 data=NS(label_transform=NS(stack_outputs=True, targets=targets)),
                 inference=NS(model=NS(head=None, select_channel=None, output_dtype=None, channel_activations=None),
                              test_time_augmentation=NS(enabled=True, rotate90_k=tk.get("rotate90_k"), ensemble_mode="mean", **{k: v for k, v in tk.items() if k != "rotate90_k"})))
        combos = mod_c.resolve_tta_augmentation_combinations(cfg.inference.test_time_augmentation, spatial_dims=3)
        plan = mod_a.build_affinity_tta_plan(cfg, augmentation_combinations=combos, num_raw=num_raw, requested_head=req)
        g = torch.Generator().manual_seed(num_raw * 7 + len(combos))
        out = []
        for i, (f, pl, k) in enumerate(combos):
            pred = torch.rand(1, num_raw, 5, 6, 6, generator=g)
            plane = pl if pl is None else tuple(int(a) - (2 if min(pl) >= 2 else 0) for a in pl)
            inv, val = mod_a.invert_view(pred, flip_axes=f, rotation_plane_spatial=plane, k=k, view_plan=None if plan is None else plan.views[i],
                                         tta_plan=plan)
            out.append((round(float(inv.double().sum()), 5), round(float((inv.double() ** 2).sum()), 5),
                        [None if v is None else [(s.start, s.stop) for s in v] for v in val.channels]))
        return (None if plan is None else sorted(plan.partial_channels)), out
    t.run("affinity TTA: plan + invert_view per view", cases, lambda *c: run(ra, rc, *c), lambda *c: run(oa, oc, *c))


def _tensor_digest(x, digits=6):
    import torch
    kind = str(x.dtype)
    x = x.detach().double()
    return (tuple(x.shape), kind, round(float(x.sum()), digits), round(float((x * x).sum()), digits), round(float(x.min()), digits),
            round(float(x.max()), digits))


def blending_maps(t, rnd):
    """The blending maps as numbers (sum / sum of squares / extrema to 1e-6): importance maps, the floored sliding maps incl. the
    distance transform, border masks."""
    import torch
    rw, ow = S.ref("connectomics.inference.window"), __import__("pytorch_connectomics_amd.inference.window", fromlist=["x"])
    rois = [(1, 1, 1), (2, 3, 3), (8, 12, 16), (112, 112, 112), (1, 32, 48), (5, 7, 9), (160, 160, 160), (3, 1, 4)] + \
        [tuple(rnd.randint(1, 40) for _ in range(3)) for _ in range(40)]
    modes = ["constant", "bump", "gaussian", "distance_transform", "dt", "BUMP", "const", "nope"]
    t.run("compute_importance_map", [(r, m) for r in rois for m in modes],
          lambda r, m: _tensor_digest(rw.compute_importance_map(r, mode=m, device="cpu", dtype=torch.float32)),
          lambda r, m: _tensor_digest(ow.compute_importance_map(r, mode=m, device="cpu", dtype=torch.float32)))
    t.run("build_sliding_importance_map", [(r, m) for r in rois for m in modes],
          lambda r, m: _tensor_digest(rw.build_sliding_importance_map(r, mode=m, device="cpu", dtype=torch.float32)),
          lambda r, m: _tensor_digest(ow.build_sliding_importance_map(r, mode=m, device="cpu", dtype=torch.float32)))
    borders = [[], [0, 0, 0], [1, 1, 1], [2, 0, 1], [50, 1, 1], [1, 1], [-1, 0, 0], None]
    t.run("apply_border_mask", [(r, b) for r in rois[:20] for b in borders],
          lambda r, b: _tensor_digest(rw.apply_border_mask(torch.ones(r) + torch.arange(r[2]), b)),
          lambda r, b: _tensor_digest(ow.apply_border_mask(torch.ones(r) + torch.arange(r[2]), b)))


def output_transforms(t, rnd):
    import numpy as np
    ro, oo = S.ref("connectomics.inference.output"), __import__("pytorch_connectomics_amd.inference.output", fromlist=["x"])
    rng = np.random.default_rng(3)
    data = [(rng.random((2, 3, 4, 5)).astype(np.float32) * s + o) for s, o in ((1.0, 0.0), (300.0, -20.0), (1e-3, 0.0), (70000.0, 0.0))]
    cases = []
    for d in data:
        for enabled in (True, False):
            for scale in (-1.0, 255.0, 1.0, 0.5, 65535.0, None):
                for idt in (None, "uint8", "uint16", "float16", "int8", "float32", "int16", "bogus"):
                    for sdt in (None, "float16", "uint8", "bogus"):
                        cases.append((NS(inference=NS(prediction_transform=NS(enabled=enabled, intensity_scale=scale, intensity_dtype=idt),
                                                      save_dtype=sdt, save_prediction=NS(storage_dtype=sdt))), d))

    def digest(a):
        a = np.asarray(a)
        return (a.shape, str(a.dtype), round(float(a.astype(np.float64).sum()), 4), float(a.min()), float(a.max()))
    t.run("apply_prediction_transform", cases, lambda c, d: digest(ro.apply_prediction_transform(c, d.copy())),
          lambda c, d: digest(oo.apply_prediction_transform(c, d.copy())))
    t.run("apply_storage_dtype_transform", cases, lambda c, d: digest(ro.apply_storage_dtype_transform(c, d.copy())),
          lambda c, d: digest(oo.apply_storage_dtype_transform(c, d.copy())))


def training_host_side(t, rnd):
    """Learning-rate schedule, optimizer parameter groups and the torch restatements of the reference's weighted losses (value and
    gradient digests) on generated configurations / tensors."""
    import torch
    import pytorch_connectomics_amd.training.module as om
    rl = S.ref("connectomics.training.optimization.lr_scheduler")
    rb = S.ref("connectomics.training.optimization.build")
    ls = S.ref("connectomics.models.losses.losses")

    def lr_curve(cls, max_iters, wi, wf, eta):
        ps = [torch.nn.Parameter(torch.zeros(1)), torch.nn.Parameter(torch.zeros(1))]
        opt = torch.optim.SGD([{"params": [ps[0]], "lr": 0.1}, {"params": [ps[1]], "lr": 0.02}], lr=0.1)
        sch = cls(opt, max_iters=max_iters, warmup_factor=wf, warmup_iters=wi, eta_min=eta)
        seq = []
        for _ in range(max_iters):
            seq.append([round(g["lr"], 12) for g in opt.param_groups])
            opt.step()
            sch.step()
        return seq
    cases = [(rnd.randint(2, 80), rnd.choice([0, 1, 5, 20, 100]), rnd.choice([1e-3, 0.1, 1.0, 0.0]), rnd.choice([0.0, 1e-6, 1e-3])) for _ in range(60)]
    t.run("WarmupCosineLR per-iteration rates", cases, lambda *c: lr_curve(rl.WarmupCosineLR, *c), lambda *c: lr_curve(om.WarmupCosineLR, *c))

    def model():
        torch.manual_seed(0)
        m = torch.nn.Sequential()
        m.add_module("conv", torch.nn.Conv3d(1, 4, 3))
        m.add_module("gn", torch.nn.GroupNorm(2, 4))
        m.add_module("act", torch.nn.PReLU())
        m.add_module("conv2", torch.nn.Conv3d(4, 4, 1, bias=False))
        m.add_module("bn", torch.nn.BatchNorm3d(4))
        m.add_module("ln", torch.nn.LayerNorm(4))
        m.add_module("head", torch.nn.Conv3d(4, 2, 1))
        m.add_module("tied", torch.nn.Conv3d(4, 2, 1))
        m.tied.weight = m.head.weight
        m.conv2.weight.requires_grad_(False)
        return m

    def groups(build, oc):
        m = model()
        opt = build(NS(optimization=NS(optimizer=NS(**oc))), m)
        names = {id(p): n for n, p in m.named_parameters()}
        per = {names[id(p)]: (g["lr"], g["weight_decay"]) for g in opt.param_groups for p in g["params"]}
        g0 = opt.param_groups[0]
        return type(opt).__name__, sorted(per.items()), g0.get("betas"), g0.get("eps"), g0.get("momentum")
    ocs = []
    for name in ("AdamW", "adamw", "Adam", "SGD", "sgd", "RMSprop", "nonsense"):
        for _ in range(6):
            oc = dict(name=name, lr=rnd.choice([1e-3, 2e-4, 0.1]), weight_decay=rnd.choice([0.0, 0.01, 0.05]))
            if rnd.random() < 0.5:
                oc.update(weight_decay_norm=rnd.choice([0.0, 0.001]), weight_decay_bias=rnd.choice([0.0, 0.02]), bias_lr_factor=rnd.choice([1.0, 2.0]))
            if rnd.random() < 0.4:
                oc.update(betas=[0.8, 0.95], eps=1e-6, momentum=0.8)
            ocs.append((oc,))
    t.run("build_optimizer per-parameter (lr, weight_decay)", ocs, lambda oc: groups(rb.build_optimizer, oc), lambda oc: groups(om.build_optimizer, oc))

    g = torch.Generator().manual_seed(77)
    def loss_digest(fn, shape, weight_kind, pos):
        x = (torch.randn(*shape, generator=g) * 3).requires_grad_(True)
        y = (torch.rand(*shape, generator=g) > 0.6).float()
        w = {None: None, "full": torch.rand(*shape, generator=g), "broadcast": torch.rand(shape[0], 1, *shape[2:], generator=g),
             "zeros": torch.zeros(*shape)}[weight_kind]
        v = fn(x, y, w, pos)
        if v.requires_grad:                 # an all-invalid weight map gives the reference a constant 0 (no graph): gradient 0 either way
            v.backward()
        return round(float(v), 6), round(float(x.grad.double().abs().sum()), 6) if x.grad is not None else 0.0
    shapes = [(2, 1, 4, 5, 6), (1, 3, 3, 4, 4), (2, 2, 6, 6)]
    lcases = [(sh, wk, pw) for sh in shapes for wk in (None, "full", "broadcast", "zeros") for pw in (None, 2.5)]
    def ref_bce(x, y, w, pos):
        return ls.WeightedBCEWithLogitsLoss(pos_weight=None if pos is None else torch.tensor(pos))(x, y, w)
    def our_bce(x, y, w, pos):
        return om.weighted_bce_with_logits(x, y, w, None if pos is None else torch.tensor(pos))
    state = {}
    def seeded(fn):
        def run(*c):
            g.manual_seed(hash(str(c)) % (2 ** 31))
            return loss_digest(fn, *c)
        return run
    t.run("WeightedBCEWithLogitsLoss value + gradient", lcases, seeded(ref_bce), seeded(our_bce))
    for kind, cls in (("mse", ls.WeightedMSELoss), ("mae", ls.WeightedMAELoss)):
        t.run(f"Weighted{kind.upper()}Loss value + gradient", [(sh, wk, None) for sh in shapes for wk in (None, "full", "broadcast")],
              seeded(lambda x, y, w, pos, cls=cls: cls()(x, y, w)), seeded(lambda x, y, w, pos, kind=kind: om.weighted_regression_loss(kind, x, y, w)))
    # ScnpLoss (losses.py:354-453) against the restatement of training/scnp_autograd.py; the reference's class slices its weight per
    # channel, so it sees a broadcast weight expanded
    from pytorch_connectomics_amd.training.scnp_autograd import ScnpLoss
    for ns in (1, 3, 5):
        t.run(f"ScnpLoss(neighborhood_size={ns}) value + gradient", [(sh, wk, None) for sh in shapes for wk in (None, "full", "broadcast")],
              seeded(lambda x, y, w, pos, ns=ns: ls.ScnpLoss(neighborhood_size=ns)(x, y, None if w is None else w.expand_as(x))),
              seeded(lambda x, y, w, pos, ns=ns: ScnpLoss(neighborhood_size=ns)(x, y, w)))
    # the regularisers (models/losses/regularization.py) against the restatements of training/regularization_autograd.py: value and the
    # gradient of every input, on generated shapes, masks and arguments
    import pytorch_connectomics_amd.training.regularization_autograd as ora
    rr = S.ref("connectomics.models.losses.regularization")

    def reg_digest(mod, name, kwargs, shape, n_in, mask_kind, seed):
        gg = torch.Generator().manual_seed(seed)
        xs = [(torch.randn(*shape, generator=gg) * 2.5).requires_grad_(True) for _ in range(n_in)]
        m = {None: None, "full": torch.rand(*shape, generator=gg), "one": torch.rand(shape[0], 1, *shape[2:], generator=gg)}[mask_kind]
        loss = getattr(mod, name)(**kwargs)
        v = loss(*xs) if m is None else loss(*xs, mask=m)
        v.backward()
        return float(v), [float(x.grad.double().abs().sum()) for x in xs]
    rshapes = [(2, 1, 3, 5, 6), (1, 1, 1, 7, 1), (1, 1, 4, 4, 9)]
    for name, n_in, kws, shs in (
            ("BinaryRegularization", 1, [{}, {"min_threshold": 0.1}, {"apply_sigmoid": False}], rshapes + [(2, 3, 4, 5)]),
            ("ForegroundDistanceConsistency", 2, [{}], rshapes + [(2, 3, 4, 5)]),
            ("ContourDistanceConsistency", 2, [{}], rshapes + [(2, 3, 4, 5)]),
            ("ForegroundContourConsistency", 2, [{}, {"eps": 1e-4}, {"kernel_half_size": 0}, {"kernel_half_size": 2}], rshapes)):
        rcases = [(name, kw, sh, n_in, mk, rnd.randint(0, 2 ** 30)) for kw in kws for sh in shs
                  for mk in ((None, "full", "one") if sh[1] > 1 else (None, "full"))]
        t.run(f"{name} value + gradients", rcases, lambda *c: reg_digest(rr, *c), lambda *c: reg_digest(ora, *c))
    t.run("NonOverlapRegularization value + gradients",
          [("NonOverlapRegularization", kw, sh, 1, None, rnd.randint(0, 2 ** 30)) for kw in ({}, {"cleft_masked": False})
           for sh in ((2, 1, 3, 4, 5), (2, 2, 3, 4, 5), (1, 3, 3, 4, 5), (2, 5, 6, 7))],
          lambda *c: reg_digest(rr, *c), lambda *c: reg_digest(ora, *c))
    # the term planner (training/losses/plan.py:126-259) against the plan ConnectomicsModule builds: call kind, slices, heads, messages
    S._stub_pkg("connectomics.training.losses")
    S._stub_pkg("connectomics.config.pipeline")
    meta = S.ref("connectomics.models.losses.metadata")
    for n in dir(meta):
        if not n.startswith("_"):
            setattr(sys.modules["connectomics.models.losses"], n, getattr(meta, n))
    plan = S.ref("connectomics.training.losses.plan")
    from pytorch_connectomics_amd.training.loss_table import LOSS_TABLE
    reg_names = sorted(n for n, row in LOSS_TABLE.items() if row.call != "pred_target")

    def plan_cfg(terms, heads):
        return NS(model=NS(loss=NS(deep_supervision=False, deep_supervision_weights=[1.0], deep_supervision_clamp_min=-20.0,
                                   deep_supervision_clamp_max=20.0, losses=terms, loss_balancing=None, fused=True),
                           primary_head=None, heads=heads, out_channels=3), data=NS(label_transform=None), optimization=NS())

    def ref_plan(terms, heads):
        mods = [meta.attach_loss_metadata(getattr(rr, tm["function"])() if tm["function"] in reg_names else ls.WeightedBCEWithLogitsLoss(),
                                          tm["function"]) for tm in terms]
        specs = plan.compile_loss_terms_from_config(plan_cfg(terms, heads), mods, [1.0] * len(terms))
        return [(s.call_kind, s.pred_slice, s.pred2_slice, s.pred_head, s.pred2_head, s.mask_slice, s.coefficient) for s in specs]

    def our_plan(terms, heads):
        m = om.ConnectomicsModule(plan_cfg(terms, heads), model=torch.nn.Identity())
        return [(s["call_kind"], s["pred_slice"], s["pred2_slice"], s["pred_head"], s["pred2_head"], s["mask_slice"], s["weight"])
                for s in m.loss_terms]
    pcases = []
    for _ in range(300):
        heads = rnd.choice([None, None, {"a": {"out_channels": 2, "target_slice": "0:2"}, "b": {"out_channels": 1, "target_slice": "2:3"}}])
        tm = {"function": rnd.choice(reg_names + ["WeightedBCEWithLogitsLoss"])}
        for key, values in (("pred_slice", ["0:1", 1]), ("pred", ["1:2"]), ("pred2_slice", ["0:1", "2:3"]), ("pred2", [0]),
                            ("mask_slice", ["3:4"]), ("mask", ["0:1"]), ("coefficient", [0.3]), ("weight", [2.0]),
                            ("pred_head", ["a", "b", "c"]), ("pred2_head", ["a", "b", "c"]), ("pos_weight", [2.0]),
                            ("call_kind", ["pred_only", "pred_pred", "pred_target", "bogus"]), ("call", ["pred_only", "pred_pred"])):
            if rnd.random() < (0.6 if key in ("pred_slice", "pred2_slice") else 0.2):
                tm[key] = rnd.choice(values)
        pcases.append(([tm], heads))
    # a term that restates ANOTHER valid kind than its loss's own is refused here when the module is built; the reference plans it and
    # fails at the first loss call
    t.run("loss term plan (call kinds, slices, heads)", pcases, ref_plan, our_plan,
          same=lambda case, a, b: b[0] == "err" and b[2].startswith("Unsupported call_kind") and
          case[0][0].get("call_kind", case[0][0].get("call")) in ("pred_target", "pred_only", "pred_pred"), show=6)


def predictor_orchestration(t, rnd):
    """TTAPredictor.predict end to end on whole images: the reference predictor (direct network, CPU tensors) against this package's
    predictor with the device kernels replaced by the torch stand-ins of tests/test_host_lazy_tta.py and a one-window engine -- which
    views run, inverse views, activation / channel selection order, per-channel ensemble modes, masks, output dtype."""
    import torch
    sys.path.insert(0, str(ROOT / "tests"))
    import test_host_distributed_inference as H
    import test_host_lazy_tta as L
    import pytorch_connectomics_amd.inference.tta as otta
    import pytorch_connectomics_amd.inference.tta_ensemble as oens
    rtta = S.ref("connectomics.inference.tta")
    otta.ops = oens.ops = L._Ops

    def net(x):
        z = torch.linspace(-1, 1, x.shape[2]).view(1, 1, -1, 1, 1)
        y = torch.linspace(-1, 1, x.shape[3]).view(1, 1, 1, -1, 1)
        w = torch.linspace(-1, 1, x.shape[4]).view(1, 1, 1, 1, -1)
        return torch.cat([x * (1.0 + 0.5 * w) + 0.25 * y, torch.tanh(2 * x - 1) * z + 0.1 * w * y, 3 * x * x - 1.5 * w + z * y], 1)
    acts = [None, [{"channels": ":", "activation": "sigmoid"}], [{"channels": "0:2", "activation": "scale_sigmoid:0.5"}, {"channels": "2", "activation": "tanh"}],
            [{"channels": ":", "activation": "softmax"}], [{"channels": "1", "activation": "tanh"}], [{"channels": "0", "activation": "none"}]]
    selects = [None, [2, 0], "0:2", 1, [1]]
    modes = ["mean", "min", "max", [["0:2", "min"], ["2", "max"]], [["0", "max"]]]
    flips = ["all", [[0], [1, 2]], None, [[2]]]
    rots = [None, [[1, 2]]]
    cases = []
    for a in acts:
        for sel in selects:
            for m in modes:
                for f in flips:
                    for r in rots:
                        if rnd.random() < 0.35:
                            cases.append((a, sel, m, f, r, rnd.random() < 0.5, rnd.choice([None, "float16"])))

    def cfg_of(a, sel, m, f, r, odt):
        return NS(model=NS(primary_head=None, heads=None, out_channels=3),
                  data=NS(train=NS(do_2d=False), val=NS(do_2d=False), dataloader=NS(batch_size=1), label_transform=None),
                  inference=NS(sliding_window=None, model=NS(head=None, select_channel=sel, output_dtype=odt, channel_activations=a, crop_pad=None),
                               test_time_augmentation=NS(enabled=True, flip_axes=f, rotation90_axes=r, rotate90_k=None, ensemble_mode=m,
                                                         patch_first_local=True, distributed_sharding=False, apply_mask=True,
                                                         empty_cache_interval=0)))
    g = torch.Generator().manual_seed(5)
    x = torch.rand(1, 1, 6, 10, 10, generator=g)
    mask = (torch.rand(1, 1, 6, 10, 10, generator=g) > 0.4).float()

    def ref_run(a, sel, m, f, r, use_mask, odt):
        p = rtta.TTAPredictor(cfg=cfg_of(a, sel, m, f, r, odt), sliding_inferer=None, forward_fn=net)
        return _tensor_digest(p.predict(x.clone(), mask=mask if use_mask else None), 4)

    class Engine(H._WholeImageEngine):
        def accumulate(self, vol, network, view=0, weight=None, add_weight=True, chan_map=None):
            from pytorch_connectomics_amd import _native as nat
            dims = [d + 2 for d, bit in enumerate((nat.VIEW_FLIP_Z, nat.VIEW_FLIP_Y, nat.VIEW_FLIP_X)) if view & bit]
            xx = vol.unsqueeze(0)
            if view & nat.VIEW_SWAP_YX:                   # the kernels' encoding: out[z, y, x] = win[T(F(z, y, x))], T = yx transpose
                xx = torch.flip(xx.transpose(3, 4), dims) if dims else xx.transpose(3, 4)
                yy = network(xx.contiguous())
                yy = (torch.flip(yy, dims) if dims else yy).transpose(3, 4)
            else:
                xx = torch.flip(xx, dims) if dims else xx
                yy = network(xx)
                yy = torch.flip(yy, dims) if dims else yy
            return yy[0].contiguous().clone(), (torch.ones(vol.shape[1:]) if weight is None else weight)

    def our_run(a, sel, m, f, r, use_mask, odt):
        p = otta.TTAPredictor(cfg=cfg_of(a, sel, m, f, r, odt), sliding_inferer=Engine(tuple(x.shape[2:])), forward_fn=net)
        p._engine_network = lambda: net
        return _tensor_digest(p.predict(x.clone(), mask=mask if use_mask else None), 4)
    def half_precision_close(case, a, b):
        """`output_dtype: float16`: the reference ENSEMBLES in the output dtype, this package ensembles in fp32 and casts once at the
        end (deviation iii) -- same shape and dtype, sums within fp16 accumulation noise."""
        if case[-1] != "float16" or a[0] != "ok" or b[0] != "ok":
            return False
        ra, rb = eval(a[1]), eval(b[1])
        return ra[0] == rb[0] and ra[1] == rb[1] == "torch.float16" and all(abs(u - v) <= 2e-3 * max(1.0, abs(u)) for u, v in zip(ra[2:], rb[2:]))
    t.run("TTAPredictor.predict (views, activations, selection, modes, mask)", cases, ref_run, our_run, same=half_precision_close)
    # a batch of two volumes (sample-wise masks), a subset of the configurations
    xb = torch.rand(2, 1, 6, 10, 10, generator=g)
    mb = (torch.rand(2, 1, 6, 10, 10, generator=g) > 0.4).float()

    def ref_batch(a, sel, m, f, r, use_mask, odt):
        p = rtta.TTAPredictor(cfg=cfg_of(a, sel, m, f, r, odt), sliding_inferer=None, forward_fn=net)
        return _tensor_digest(p.predict(xb.clone(), mask=mb if use_mask else None), 4)

    def our_batch(a, sel, m, f, r, use_mask, odt):
        p = otta.TTAPredictor(cfg=cfg_of(a, sel, m, f, r, odt), sliding_inferer=Engine(tuple(xb.shape[2:])), forward_fn=net)
        p._engine_network = lambda: net
        return _tensor_digest(p.predict(xb.clone(), mask=mb if use_mask else None), 4)
    t.run("TTAPredictor.predict on a batch of two volumes", cases[::6], ref_batch, our_batch, same=half_precision_close)

    # directional-affinity outputs, whole-volume views (`patch_first_local: false`): inverse views re-anchor the affinity channels,
    # the ensemble counts only the voxels a view really covers
    unit = ["1-0-0", "0-1-0", "0-0-1"]
    acases = []
    for offs in (unit, unit + ["3-0-0", "0-3-0", "0-0-3"], unit + ["2-0-0", "0-4-0", "0-0-4"]):
        for amode in ("deepem", "banis"):
            for f, r in (("all", None), ([[0]], [[1, 2]]), ([[1], [2]], None), (None, [[1, 2]]), ("all", [[1, 2]])):
                for m in ("mean", "min", "max"):
                    for sel in (None, "0:3", [2, 0]):
                        if rnd.random() < 0.5:
                            acases.append((offs, amode, f, r, m, sel, rnd.random() < 0.4))

    def acfg(offs, amode, f, r, m, sel):
        c = cfg_of([{"channels": ":", "activation": "sigmoid"}], sel, m, f, r, None)
        c.model.out_channels = len(offs)
        c.data.label_transform = NS(stack_outputs=True, targets=[{"name": "affinity", "kwargs": {"offsets": offs, "affinity_mode": amode}}])
        c.inference.test_time_augmentation.patch_first_local = False
        return c
    xa = torch.rand(1, 1, 6, 8, 8, generator=g)
    ma = (torch.rand(1, 1, 6, 8, 8, generator=g) > 0.4).float()

    def anet(n):
        def fn(x):
            w = torch.linspace(-1, 1, x.shape[4]).view(1, 1, 1, 1, -1)
            z = torch.linspace(-1, 1, x.shape[2]).view(1, 1, -1, 1, 1)
            return torch.cat([x * (1.0 + 0.3 * i) + 0.2 * w * (i % 2) + 0.1 * z * i for i in range(n)], 1)
        return fn

    def aref(offs, amode, f, r, m, sel, use_mask):
        p = rtta.TTAPredictor(cfg=acfg(offs, amode, f, r, m, sel), sliding_inferer=None, forward_fn=anet(len(offs)))
        return _tensor_digest(p.predict(xa.clone(), mask=ma if use_mask else None), 4)

    def aours(offs, amode, f, r, m, sel, use_mask):
        fn = anet(len(offs))
        p = otta.TTAPredictor(cfg=acfg(offs, amode, f, r, m, sel), sliding_inferer=Engine(tuple(xa.shape[2:])), forward_fn=fn)
        p._engine_network = lambda: fn
        return _tensor_digest(p.predict(xa.clone(), mask=ma if use_mask else None), 4)
    t.run("TTAPredictor.predict, affinity outputs, whole-volume views", acases, aref, aours)


def model_builders(t, rnd):
    """`build_rsunet` / `build_rsunet_iso` over generated model configurations: state-dict keys, shapes and dtypes, buffers, the
    model-info dictionary and constructor errors of the reference RSUNet against this package's (a checkpoint of one loads into the
    other with strict=True iff these agree).  MedNeXt / MONAI builders need packages the image lacks on the reference side."""
    rr = S.ref("connectomics.models.architectures.rsunet")
    import pytorch_connectomics_amd.models.architectures.rsunet as orr

    def describe(mod, builder, cfg):
        m = getattr(mod, builder)(cfg)
        sd = m.state_dict()
        info = m.get_model_info() if hasattr(m, "get_model_info") else {}
        return (sorted((k, tuple(v.shape), str(v.dtype)) for k, v in sd.items()),
                {k: info.get(k) for k in ("parameters", "trainable_parameters", "deep_supervision", "output_scales")})
    widths = [[8, 16], [16, 32, 64, 128], [6, 8, 12], [4], [4, 4, 4, 4, 4], [16, 16]]
    cases = []
    for w in widths:
        for norm in ("batch", "group", "instance", "none", "layer", "weird"):
            for act in ("relu", "elu", "leaky_relu", "prelu", "gelu", "bogus"):
                if rnd.random() > 0.35:
                    continue
                depth = len(w) - 1
                down = rnd.choice([None, [[1, 2, 2]] * depth, [[2, 2, 2]] * depth, [[1, 2, 2]] * max(0, depth - 1)])
                rs = NS(width=w, norm=norm, activation=act, num_groups=rnd.choice([2, 4, 8, 3]), down_factors=down,
                        depth_2d=rnd.choice([0, 1, 2]), kernel_2d=rnd.choice([None, [1, 3, 3], [1, 5, 5]]),
                        act_negative_slope=0.05, act_init=0.1)
                cfg = NS(model=NS(in_channels=rnd.choice([1, 2]), out_channels=rnd.choice([1, 3]), rsunet=rs,
                                  loss=NS(deep_supervision=rnd.random() < 0.4)))
                cases.append((rnd.choice(["build_rsunet", "build_rsunet_iso"]), cfg))
    t.run("build_rsunet / build_rsunet_iso: state dict + model info", cases, lambda b, c: describe(rr, b, c), lambda b, c: describe(orr, b, c))


def lazy_accessor_geometry(t, rnd):
    """The disk-backed volume reader on generated geometries: the REFERENCE's LazyVolumeAccessor (HDF5 through the in-repo libhdf5
    shim standing in for h5py, its real smart_normalize / grid_sample path) against this package's accessor (raw storage box + index
    tables, executed by the numpy restatement of the device kernels, oracle/accessor_oracle.py): shapes, a window that overhangs
    the volume, the full volume.  Values to 1e-3 of the range (trilinear weights travel through a normalised grid in the reference)."""
    import tempfile
    import types
    import numpy as np
    from oracle import accessor_oracle as AO
    from pytorch_connectomics_amd.inference.lazy_accessor import LazyVolumeAccessor
    from pytorch_connectomics_amd.utils import h5lite
    if not h5lite.available():
        print("lazy accessor geometry: skipped (libpytc_h5.so not built)")
        return
    sys.modules["h5py"] = h5lite
    for name in ("imageio", "cv2"):
        sys.modules.setdefault(name, types.ModuleType(name))
    for name in ("connectomics.data.augmentation.augment_ops", "connectomics.data.io.io", "connectomics.inference.lazy"):
        sys.modules.pop(name, None)
    lz = S.ref("connectomics.inference.lazy")
    rng = np.random.default_rng(11)
    cases = []
    with tempfile.TemporaryDirectory() as d:
        vols = {"u8": (rng.random((9, 11, 13)) * 255).astype(np.uint8), "f32c": rng.random((2, 8, 10, 12)).astype(np.float32),
                "u16last": (rng.random((8, 9, 10, 3)) * 900).astype(np.uint16)}
        paths = {}
        for k, v in vols.items():
            paths[k] = str(Path(d) / f"{k}.h5")
            with h5lite.File(paths[k], "w") as fh:
                fh.create_dataset("main", data=v, compression="gzip")
        for i in range(70):
            key = rnd.choice(list(vols))
            kind = rnd.choice(["image", "image", "mask"])
            kw = dict(kind=kind)
            if rnd.random() < 0.5:
                kw["transpose_axes"] = tuple(rnd.sample([0, 1, 2], 3))
            if rnd.random() < 0.5:
                kw["scale_factors"] = tuple(rnd.choice([0.5, 0.75, 1.0, 1.25, 1.5, 2.0]) for _ in range(3))
            if rnd.random() < 0.6:
                kw["context_pad"] = tuple((rnd.randint(0, 3), rnd.randint(0, 3)) for _ in range(3))
                kw["context_pad_mode"] = rnd.choice(["constant", "reflect", "edge", "replicate"]) if kind == "image" else "constant"
            if kind == "image":
                kw["normalize_mode"] = rnd.choice(["none", "0-1", "normal", "divide-255", "divide-2.5"])
                if kw["normalize_mode"] != "none" and rnd.random() < 0.4:
                    kw["clip_percentile_low"], kw["clip_percentile_high"] = 0.05, 0.95
            else:
                kw["binarize"], kw["threshold"] = True, rnd.choice([0.3, 100.0])
            # windows that overhang the volume but always intersect it (a window entirely outside has no defined result in the
            # reference: it returns a zero-extent array)
            loc = tuple(rnd.randint(-2, 2) for _ in range(3))
            size = tuple(rnd.randint(4, 8) for _ in range(3))
            outer = rnd.choice(["constant", "reflect", "replicate"])
            cases.append((paths[key], kw, loc, size, outer))

        def digest(a):
            a = np.asarray(a, dtype=np.float64)
            span = max(1.0, float(np.abs(a).max()))
            return (a.shape, round(float(a.sum()) / span / max(1, a.size) * 1e3), round(float(np.abs(a).sum()) / span / max(1, a.size) * 1e3))

        def ref_run(path, kw, loc, size, outer):
            with lz.LazyVolumeAccessor(path, **kw) as acc:
                shapes = [acc.channel_count, *acc.raw_spatial_shape, *acc.logical_spatial_shape, *acc.transformed_spatial_shape, *acc.padded_spatial_shape]
                return shapes, digest(acc.read_patch(loc, size, outer_pad_mode=outer, outer_pad_value=0.25)), digest(acc.load_full())

        def our_run(path, kw, loc, size, outer):
            with LazyVolumeAccessor(path, **kw) as acc:
                shapes = [acc.channel_count, *acc.raw_spatial_shape, *acc.logical_spatial_shape, *acc.transformed_spatial_shape, *acc.padded_spatial_shape]
                return shapes, digest(AO.read_patch(acc, loc, size, outer_pad_mode=outer, outer_pad_value=0.25)), digest(AO.load_full(acc))
        t.run("LazyVolumeAccessor geometry (transpose / resize / pad / normalise / window)", cases, ref_run, our_run)


def lazy_engine(t, rnd):
    """The lazy region / volume engine end to end on generated configurations (blending mode, per-axis overlap, snapped grids, target
    context, regions, per-window TTA, mask volumes, activations, channel selection): the REFERENCE's lazy loop on numpy-backed
    accessors against this package's loop with the device kernels replaced by torch stand-ins (tests/test_host_lazy_tta.py)."""
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT / "tests"))
    import test_host_lazy_tta as L
    import pytorch_connectomics_amd.inference.lazy as ol
    import pytorch_connectomics_amd.inference.tta as otta
    import pytorch_connectomics_amd.inference.tta_ensemble as oens
    ol.ops = otta.ops = oens.ops = L._Ops
    for name in ("connectomics.inference.lazy",):
        sys.modules.pop(name, None)
    lz = S.ref("connectomics.inference.lazy")
    rng = np.random.default_rng(19)
    vol = rng.random((1, 14, 22, 26), dtype=np.float32)
    mask = (rng.random((1, 14, 22, 26)) > 0.4).astype(np.float32)

    class Fake:
        def __init__(self, v, kind):
            self.vol, self.kind = v, kind
            self.padded_spatial_shape, self.channel_count = tuple(v.shape[1:]), v.shape[0]

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def close(self):
            pass

        def read_patch(self, location, patch_size, *, outer_pad_mode, outer_pad_value):
            start = tuple(int(v) for v in location)
            end = tuple(start[i] + int(patch_size[i]) for i in range(3))
            shp = self.padded_spatial_shape
            lo = tuple(max(0, start[i]) for i in range(3))
            hi = tuple(min(shp[i], end[i]) for i in range(3))
            pads = [(max(0, -start[i]), max(0, end[i] - shp[i])) for i in range(3)]
            return lz._pad_channel_first(self.vol[:, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]], pads, mode=outer_pad_mode, constant_value=outer_pad_value)
    lz._build_accessor = lambda cfg_, path, kind, mode: Fake(mask if kind == "mask" else vol, kind)

    def net(x):
        ramp = torch.linspace(0, 1, x.shape[-1]).view(1, 1, 1, 1, -1)
        shifted = torch.zeros_like(x)
        shifted[..., 1:, :, :] = x[..., :-1, :, :]
        return torch.cat([2 * x - 1 + ramp, 0.5 * x + shifted], 1)
    cases = []
    for _ in range(70):
        roi = rnd.choice([(6, 8, 8), (4, 6, 10), (8, 8, 8), (5, 7, 9)])
        ctx = rnd.choice([[], [], [1, 1, 1], [0, 2, 1]])
        tta = rnd.random() < 0.5
        kw = dict(roi=roi, blending=rnd.choice(["bump", "constant", "gaussian", "distance_transform"]),
                  overlap=rnd.choice([0.5, 0.25, 0.0, [0.25, 0.5, 0.5]]), snap=rnd.random() < 0.4, ctx=ctx,
                  padding_mode=rnd.choice(["constant", "reflect", "replicate"]), swb=rnd.choice([1, 3, 4]),
                  acts=rnd.choice([None, [{"channels": "0", "activation": "sigmoid"}], [{"channels": ":", "activation": "tanh"}]]),
                  select=rnd.choice([None, [1], "0:1"]), tta=tta, flips=rnd.choice(["all", [[0]], [[1, 2]]]) if tta else None,
                  mode=rnd.choice(["mean", "min", "max"]))
        region = None
        if rnd.random() < 0.4:
            lo = tuple(rnd.randint(0, d - 3) for d in vol.shape[1:])
            region = (lo, tuple(rnd.randint(l + 2, d) for l, d in zip(lo, vol.shape[1:])))
        cases.append((kw, region, rnd.random() < 0.4))

    def cfg_of(kw):
        return NS(model=NS(primary_head=None, heads=None, out_channels=2, output_size=list(kw["roi"])), system=NS(num_workers=0),
                  data=NS(train=NS(do_2d=False), val=NS(do_2d=False), dataloader=NS(batch_size=1, use_lazy_zarr=False, use_lazy_h5=False), label_transform=None),
                  inference=NS(sliding_window=NS(window_size=list(kw["roi"]), sw_batch_size=kw["swb"], overlap=kw["overlap"], blending=kw["blending"],
                                                 padding_mode=kw["padding_mode"], cval=0.0, keep_input_on_cpu=False, sw_device=None, output_device=None,
                                                 border_mask=[], distributed_sharding=False, snap_to_edge=kw["snap"], target_context=list(kw["ctx"]),
                                                 distributed_reduce_chunk_mb=128),
                               model=NS(head=None, select_channel=kw["select"], output_dtype=None, channel_activations=kw["acts"], crop_pad=None),
                               test_time_augmentation=NS(enabled=kw["tta"], distributed_sharding=False, flip_axes=kw["flips"], rotation90_axes=None,
                                                         rotate90_k=None, ensemble_mode=kw["mode"], patch_first_local=True, apply_mask=True,
                                                         empty_cache_interval=0)))

    def run(mod, source, mask_arg, kw, region, use_mask):
        cfg = cfg_of(kw)
        extra = dict(mask_path=mask_arg if use_mask else None, device="cpu")
        if region is None:
            y = mod.lazy_predict_volume(cfg, net, source, **extra)
        else:
            y = mod.lazy_predict_region(cfg, net, source, region_start=region[0], region_stop=region[1], **extra)
        return _tensor_digest(y, 3)
    t.run("lazy engine end to end (grid, blending, context, regions, TTA, masks)", cases,
          lambda kw, region, use_mask: run(lz, "fake://", "fake://mask", kw, region, use_mask),
          lambda kw, region, use_mask: run(ol, vol, mask, kw, region, use_mask))

    # networks that break the window contract (lazy.py:389-419 `_crop_prediction_to_roi`, the tensor / mapping checks around it)
    bad_nets = {
        "smaller": lambda x: net(x)[..., 1:, :, :],
        "larger": lambda x: torch.nn.functional.pad(net(x), (1, 1, 0, 0, 0, 0)),
        "mapping": lambda x: {"output": net(x)},
        "deep_supervision": lambda x: {"output": net(x), "ds_1": net(x)[..., ::2, ::2, ::2]},
        "named_heads": lambda x: {"output": {"a": net(x), "b": net(x)}},
        "not_a_tensor": lambda x: [net(x)],
        "rank4": lambda x: net(x)[0],
        "no_batch_match": lambda x: net(x)[:1],
    }

    def run_bad(mod, source, which, ctx, tta):
        kw = dict(roi=(6, 8, 8), blending="bump", overlap=0.5, snap=False, ctx=ctx, padding_mode="reflect", swb=2, acts=None, select=None, tta=tta,
                  flips=[[0]] if tta else None, mode="mean")
        y = mod.lazy_predict_volume(cfg_of(kw), bad_nets[which], source, mask_path=None, device="cpu")
        return _tensor_digest(y, 3)
    t.run("lazy engine: networks that break the window contract", [(w, c, tt) for w in bad_nets for c in ([], [1, 1, 1]) for tt in (False, True)],
          lambda w, c, tt: run_bad(lz, "fake://", w, c, tt), lambda w, c, tt: run_bad(ol, vol, w, c, tt), show=12,
          # a network that drops samples fails in both, by accident in the reference (a broadcast error of its accumulation) and in the
          # stand-in kernels here; the product refuses it by name in hip_ops.blend_accumulate
          same=lambda case, a, b: case[0] == "no_batch_match" and a[0] == b[0] == "err")


def chunked_runner(t, rnd):
    """`run_chunked_prediction_inference` end to end on generated chunk geometries (chunk size, halo, z slabs, global crop, per-window
    TTA, mask volume, prediction transform / storage dtype): the reference runner (streams into one HDF5 through the libhdf5 shim)
    against this package's (chunk files + stitch; device kernels replaced by the torch stand-ins) -- the stitched `main` array."""
    import tempfile
    import types
    import numpy as np
    import torch
    from pytorch_connectomics_amd.utils import h5lite
    if not h5lite.available():
        print("chunked runner: skipped (libpytc_h5.so not built)")
        return
    sys.path.insert(0, str(ROOT / "tests"))
    import test_host_lazy_tta as L
    import pytorch_connectomics_amd.inference.chunked as oc
    import pytorch_connectomics_amd.inference.lazy as ol
    import pytorch_connectomics_amd.inference.tta as otta
    import pytorch_connectomics_amd.inference.tta_ensemble as oens
    ol.ops = otta.ops = oens.ops = L._Ops
    sys.modules["h5py"] = h5lite
    for name in ("imageio", "cv2"):
        sys.modules.setdefault(name, types.ModuleType(name))
    for name in ("connectomics.data.io.io", "connectomics.data.augmentation.augment_ops", "connectomics.inference.lazy", "connectomics.inference.chunked"):
        sys.modules.pop(name, None)
    rc, lz = S.ref("connectomics.inference.chunked"), S.ref("connectomics.inference.lazy")
    rng = np.random.default_rng(23)
    vol = rng.random((1, 14, 22, 26), dtype=np.float32)
    mask = (rng.random((1, 14, 22, 26)) > 0.4).astype(np.float32)

    class Fake:
        def __init__(self, v, kind):
            self.vol, self.kind = v, kind
            self.padded_spatial_shape = self.transformed_spatial_shape = tuple(v.shape[1:])
            self.channel_count = v.shape[0]

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def close(self):
            pass

        def read_patch(self, location, patch_size, *, outer_pad_mode, outer_pad_value):
            start = tuple(int(v) for v in location)
            end = tuple(start[i] + int(patch_size[i]) for i in range(3))
            shp = self.padded_spatial_shape
            lo = tuple(max(0, start[i]) for i in range(3))
            hi = tuple(min(shp[i], end[i]) for i in range(3))
            pads = [(max(0, -start[i]), max(0, end[i] - shp[i])) for i in range(3)]
            return lz._pad_channel_first(self.vol[:, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]], pads, mode=outer_pad_mode, constant_value=outer_pad_value)
    lz._build_accessor = lambda cfg_, path, kind, mode: Fake(mask if kind == "mask" else vol, kind)

    def net(x):
        ramp = torch.linspace(0, 1, x.shape[-1]).view(1, 1, 1, 1, -1)
        return torch.cat([2 * x - 1 + ramp, 0.5 * x + x.mean(dim=(2, 3, 4), keepdim=True)], 1)

    def cfg_of(kw):
        roi = kw["roi"]
        return NS(model=NS(primary_head=None, heads=None, out_channels=2, output_size=list(roi)), system=NS(num_workers=0),
                  data=NS(train=NS(do_2d=False), val=NS(do_2d=False), dataloader=NS(batch_size=1, use_lazy_zarr=False, use_lazy_h5=False, patch_size=None),
                          label_transform=None),
                  inference=NS(save_backend="h5", save_compression="gzip",
                               sliding_window=NS(window_size=list(roi), sw_batch_size=3, overlap=0.5, blending=kw["blending"], padding_mode="reflect", cval=0.0,
                                                 keep_input_on_cpu=False, sw_device=None, output_device=None, border_mask=[], distributed_sharding=False,
                                                 snap_to_edge=False, target_context=[], distributed_reduce_chunk_mb=128),
                               model=NS(head=None, select_channel=kw["select"], output_dtype=None, channel_activations=[{"channels": "0", "activation": "sigmoid"}],
                                        crop_pad=kw["crop"]),
                               prediction_transform=NS(enabled=kw["scale"] is not None, intensity_scale=kw["scale"] or -1.0, intensity_dtype=kw["idt"]),
                               save_dtype=kw["sdt"],
                               chunking=NS(enabled=True, chunk_size=list(kw["chunk"]), halo=list(kw["halo"]), axes=kw["axes"], output_mode="raw_prediction",
                                           shard_id=None, num_shards=None, roi=None, temp_dir="", save_intermediate=False, precomputed=False),
                               test_time_augmentation=NS(enabled=kw["flips"] is not None, distributed_sharding=False, flip_axes=kw["flips"], rotation90_axes=None,
                                                         rotate90_k=None, ensemble_mode="mean", patch_first_local=True, apply_mask=True, empty_cache_interval=0)))
    cases = []
    for _ in range(40):
        cases.append((dict(roi=rnd.choice([(6, 8, 8), (4, 6, 10)]), blending=rnd.choice(["bump", "constant"]), select=rnd.choice([None, [1]]),
                           crop=rnd.choice([None, None, [1, 0, 2, 1, 0, 3], [1, 1, 2]]), scale=rnd.choice([None, 255.0]), idt=rnd.choice([None, "uint8"]),
                           sdt=rnd.choice([None, "float16"]), chunk=(rnd.randint(3, 16), rnd.randint(4, 24), rnd.randint(4, 28)),
                           halo=(rnd.randint(0, 3), rnd.randint(0, 4), rnd.randint(0, 4)), axes=rnd.choice(["all", "all", "z"]),
                           flips=rnd.choice([None, None, [[0]], [[1, 2]]])), rnd.random() < 0.35))

    def digest(a):
        a = np.asarray(a)
        return (a.shape, str(a.dtype), round(float(a.astype(np.float64).sum()), 2), float(a.min()), float(a.max()))

    def ref_run(kw, use_mask):
        with tempfile.TemporaryDirectory() as d:
            out = rc.run_chunked_prediction_inference(cfg_of(kw), net, "fake://", output_path=Path(d) / "pred.h5", device="cpu",
                                                      mask_path="fake://mask" if use_mask else None)
            with h5lite.File(str(out), "r") as fh:
                return digest(fh["main"][...])

    def our_run(kw, use_mask):
        with tempfile.TemporaryDirectory() as d:
            out = oc.run_chunked_prediction_inference(cfg_of(kw), net, image_path=vol, output_path=Path(d) / "pred.h5", device="cpu",
                                                      mask_path=mask if use_mask else None)
            return digest(out)
    t.run("run_chunked_prediction_inference (chunk geometry, crop, TTA, mask, dtypes)", cases, ref_run, our_run)


def loss_orchestration(t, rnd):
    """The training loss as the reference's LossOrchestrator assembles it (training/losses/orchestrator.py:500-890, plan.py) against
    ConnectomicsModule._compute_loss (unfused path, CPU tensors): term lists over the torch-only losses with coefficients, pred /
    target / mask slices, pos_weight (default, 'auto', numeric), batch masks, deep supervision and `apply_deep_supervision` --
    total loss and the gradient of every output scale."""
    import warnings
    import torch
    warnings.filterwarnings("ignore")
    S._stub_pkg("connectomics.training.losses")
    S._stub_pkg("connectomics.config.pipeline")
    meta = S.ref("connectomics.models.losses.metadata")
    ml = sys.modules["connectomics.models.losses"]
    for n in dir(meta):
        if not n.startswith("_"):
            setattr(ml, n, getattr(meta, n))
    ls = S.ref("connectomics.models.losses.losses")
    orch = S.ref("connectomics.training.losses.orchestrator")
    from pytorch_connectomics_amd.training.module import ConnectomicsModule

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x):
            return x
    make = {"WeightedBCEWithLogitsLoss": lambda kw: ls.WeightedBCEWithLogitsLoss(**kw), "WeightedMSELoss": lambda kw: ls.WeightedMSELoss(**kw),
            "WeightedMAELoss": lambda kw: ls.WeightedMAELoss(**kw), "SmoothL1Loss": lambda kw: ls.SmoothL1Loss(**kw),
            "PerChannelBCEWithLogitsLoss": lambda kw: ls.PerChannelBCEWithLogitsLoss(**kw),
            "BCEWithLogitsLoss": lambda kw: torch.nn.BCEWithLogitsLoss(**kw), "MSELoss": lambda kw: torch.nn.MSELoss(**kw)}
    weight_taking = {"WeightedBCEWithLogitsLoss", "WeightedMSELoss", "WeightedMAELoss", "SmoothL1Loss", "PerChannelBCEWithLogitsLoss"}
    cases = []
    for _ in range(160):
        terms = []
        for _k in range(rnd.randint(1, 3)):
            fn = rnd.choice(list(make))
            term = {"function": fn, "weight": rnd.choice([1.0, 0.5, 2.0])}
            term["target_slice"] = "0:3"                 # labels carry a 4th channel (a term-mask candidate); the network has 3
            if rnd.random() < 0.4:
                term["pred_slice"], term["target_slice"] = rnd.choice([("0:1", "0:1"), ("1:3", "1:3"), ("0:2", "1:3")])
            if fn in weight_taking and rnd.random() < 0.4:
                term["pos_weight"] = rnd.choice(["auto", 2.5, 1.0])
            if rnd.random() < 0.25 and fn != "PerChannelBCEWithLogitsLoss":      # (the reference's per-channel BCE cannot take a 1-channel mask)
                term["mask_slice"] = "3:4"
            if rnd.random() < 0.2:
                term["apply_deep_supervision"] = False
            if fn == "SmoothL1Loss" and rnd.random() < 0.5:
                term["kwargs"] = {"beta": 0.5}
            terms.append(term)
        cases.append((terms, rnd.random() < 0.5, rnd.random() < 0.5, rnd.randint(0, 10 ** 6)))

    def cfg_of(terms, ds):
        return NS(model=NS(loss=NS(deep_supervision=ds, deep_supervision_weights=[1.0, 0.5, 0.25, 0.125, 0.0625], deep_supervision_clamp_min=-20.0,
                                   deep_supervision_clamp_max=20.0, losses=terms, loss_balancing=None, fused=False),
                           primary_head=None, heads=None, out_channels=3), data=NS(label_transform=None))

    def tensors(seed):
        g = torch.Generator().manual_seed(seed)
        outs = {"output": torch.randn(2, 3, 8, 8, 8, generator=g) * 6, "ds_1": torch.randn(2, 3, 4, 4, 4, generator=g) * 6}
        lab = (torch.rand(2, 4, 8, 8, 8, generator=g) > 0.7).float()
        lab[:, 2] = torch.rand(2, 8, 8, 8, generator=g)
        lab[:, 3] = (torch.rand(2, 8, 8, 8, generator=g) > 0.3).float()
        return outs, lab, (torch.rand(2, 1, 8, 8, 8, generator=g) > 0.3).float()

    def digest(total, outs):
        total.backward()
        return (round(float(total.detach()), 5),) + tuple(round(float(v.grad.double().abs().sum()), 4) if v.grad is not None else None for v in outs.values())

    def ref_run(terms, ds, use_mask, seed):
        cfg = cfg_of(terms, ds)
        mods = torch.nn.ModuleList([make[t["function"]](dict(t.get("kwargs", {}))) for t in terms])
        o = orch.LossOrchestrator(cfg, mods, [t["weight"] for t in terms], enable_nan_detection=False, debug_on_nan=False, resolve_affinity_mode_fn=lambda c: None)
        outs, lab, mask = tensors(seed)
        outs = {k: v.requires_grad_(True) for k, v in outs.items()}
        if ds:
            total, _ = o.compute_deep_supervision_loss(outs, lab, stage="train", mask=mask if use_mask else None)
        else:
            total, _ = o.compute_standard_loss(outs["output"], lab, stage="train", mask=mask if use_mask else None)
        return digest(total, outs)

    def our_run(terms, ds, use_mask, seed):
        m = ConnectomicsModule(cfg_of(terms, ds), model=Tiny())
        outs, lab, mask = tensors(seed)
        outs = {k: v.requires_grad_(True) for k, v in outs.items()}
        total, _ = m._compute_loss(outs if ds else outs["output"], lab, mask if use_mask else None)
        return digest(total, outs)
    def close(case, a, b):
        if a[0] != "ok" or b[0] != "ok":
            return False
        ra, rb = eval(a[1]), eval(b[1])
        return len(ra) == len(rb) and all((u is None and v is None) or (u is not None and v is not None and abs(u - v) <= 2e-5 * max(1.0, abs(u)))
                                          for u, v in zip(ra, rb))
    t.run("loss orchestration (terms, slices, pos_weight, masks, deep supervision)", cases, ref_run, our_run, same=close)

    # named heads: every term reads its head (pred_head / primary head), its target channels default to the head's target_slice
    heads = {"aff": {"out_channels": 2, "target_slice": "0:2"}, "sdt": {"out_channels": 1, "target_slice": "2:3"}}
    hcases = []
    for _ in range(80):
        terms = []
        for _k in range(rnd.randint(1, 3)):
            head = rnd.choice(["aff", "sdt", None])
            fn = rnd.choice(["WeightedBCEWithLogitsLoss", "WeightedMSELoss", "SmoothL1Loss"])
            term = {"function": fn, "weight": rnd.choice([1.0, 0.5])}
            if head is not None:
                term["pred_head"] = head
            if rnd.random() < 0.3:
                term["target_slice"] = "2:3" if head == "sdt" else "0:2"
            if fn != "WeightedBCEWithLogitsLoss" and rnd.random() < 0.3:
                term["pos_weight"] = rnd.choice(["auto", 3.0])
            terms.append(term)
        hcases.append((terms, rnd.choice(["aff", "sdt", None]), rnd.random() < 0.5, rnd.randint(0, 10 ** 6)))

    def hcfg(terms, primary):
        c = cfg_of(terms, False)
        c.model.heads, c.model.primary_head, c.model.out_channels = heads, primary, 3
        return c

    def htensors(seed):
        g = torch.Generator().manual_seed(seed)
        outs = {"aff": torch.randn(2, 2, 6, 6, 6, generator=g) * 4, "sdt": torch.randn(2, 1, 6, 6, 6, generator=g) * 4}
        lab = (torch.rand(2, 3, 6, 6, 6, generator=g) > 0.6).float()
        lab[:, 2] = torch.rand(2, 6, 6, 6, generator=g) * 2 - 1
        return outs, lab, (torch.rand(2, 1, 6, 6, 6, generator=g) > 0.3).float()

    def href(terms, primary, use_mask, seed):
        cfg = hcfg(terms, primary)
        mods = torch.nn.ModuleList([make[t["function"]](dict(t.get("kwargs", {}))) for t in terms])
        o = orch.LossOrchestrator(cfg, mods, [t["weight"] for t in terms], enable_nan_detection=False, debug_on_nan=False, resolve_affinity_mode_fn=lambda c: None)
        outs, lab, mask = htensors(seed)
        outs = {k: v.requires_grad_(True) for k, v in outs.items()}
        total, _ = o.compute_standard_loss({"output": outs}, lab, stage="train", mask=mask if use_mask else None)
        return digest(total, outs)

    def hours(terms, primary, use_mask, seed):
        m = ConnectomicsModule(hcfg(terms, primary), model=Tiny())
        outs, lab, mask = htensors(seed)
        outs = {k: v.requires_grad_(True) for k, v in outs.items()}
        total, _ = m._compute_loss({"output": outs}, lab, mask if use_mask else None)
        return digest(total, outs)
    t.run("loss orchestration on named heads (pred_head, primary head, head target slices)", hcases, href, hours, same=close)


def output_files(t, rnd):
    """Per-volume output naming and the HDF5 writer: `resolve_output_filenames` over generated batch metadata (the stem rule of
    runtime/output_naming.py) and `write_outputs` (directory layout, dataset name, storage dtype) -- the reference's functions with
    the libhdf5 shim standing in for h5py."""
    import tempfile
    import types
    import numpy as np
    from pytorch_connectomics_amd.utils import h5lite
    sys.modules["h5py"] = h5lite
    for name in ("imageio", "cv2"):
        sys.modules.setdefault(name, types.ModuleType(name))
    S.install()
    S._stub_pkg("connectomics.runtime")
    for name in ("connectomics.data.io.io", "connectomics.inference.output"):
        sys.modules.pop(name, None)
    ro = S.ref("connectomics.inference.output")
    io_real = S.ref("connectomics.data.io.io")                     # the reference's own HDF5 writer, on the libhdf5 shim
    for name in ("write_hdf5", "save_volume"):
        setattr(sys.modules["connectomics.data.io"], name, getattr(io_real, name))
    import pytorch_connectomics_amd.inference.output as oo
    paths = ["/data/seed101/data.zarr/img", "/data/seed101/img.h5", "/data/sample.h5", "/data/seed101/raw_aff.h5", "img.tif", "/em/raw/main.h5",
             "/a/b.n5/data/raw", "relative/vol_07.nii.gz", "/x/y/Image.PNG", "", "/", "/data/.zarr/img", "C:/weird path/em.h5", "/data/vol.ome.zarr/0"]
    cases = []
    for _ in range(300):
        n = rnd.randint(1, 3)
        picks = [rnd.choice(paths) for _ in range(n)]
        style = rnd.choice(["meta_list", "meta_dict_list", "meta_dict_one", "image_paths", "image_one", "none", "partial"])
        batch = {"image": np.zeros((n, 1, 2, 2, 2), np.float32)}
        if style == "meta_list":
            batch["image_meta_dict"] = [{"filename_or_obj": p} for p in picks]
        elif style == "meta_dict_list":
            batch["image_meta_dict"] = {"filename_or_obj": picks}
        elif style == "meta_dict_one":
            batch["image_meta_dict"] = {"filename_or_obj": picks[0]}
        elif style == "image_paths":
            batch["image"] = picks
        elif style == "image_one":
            batch["image"] = picks[0]
        elif style == "partial":
            batch["image_meta_dict"] = [{"filename_or_obj": picks[0]}, {"other": 1}, None][:n]
        cases.append((batch, rnd.randint(0, 9)))
    t.run("resolve_output_filenames", cases, lambda b, g: ro.resolve_output_filenames(None, b, g), lambda b, g: oo.resolve_output_filenames(None, b, g))

    rng = np.random.default_rng(4)
    wcases = []
    for _ in range(40):
        n = rnd.randint(1, 3)
        shape = rnd.choice([(n, 2, 3, 4, 5), (n, 1, 3, 4, 5), (n, 3, 4, 5), (3, 4, 5), (4, 5)])
        wcases.append((rng.random(shape).astype(np.float32), [f"vol{i}" for i in range(rnd.choice([n, n, max(1, n - 1)]))],
                       rnd.choice(["prediction.h5", "prediction", "decoded.seg.h5", "x.nii.gz"]), rnd.choice([None, "float16", "uint8"])))

    def written(mod, preds, names, suffix, sdt):
        with tempfile.TemporaryDirectory() as d:
            cfg = NS(inference=NS(save_path=d, save_backend="h5", save_dtype=sdt), data=NS(nnunet_preprocessing=None))
            mod.write_outputs(cfg, preds.copy(), list(names), suffix=suffix, mode="test")
            out = []
            for f in sorted(Path(d).rglob("*")):
                if f.is_file():
                    with h5lite.File(str(f), "r") as fh:
                        a = np.asarray(fh["main"][...])
                    out.append((str(f.relative_to(d)), a.shape, str(a.dtype), round(float(a.astype(np.float64).sum()), 3)))
            return out
    t.run("write_outputs (layout, dataset, storage dtype)", wcases, lambda *c: written(ro, *c), lambda *c: written(oo, *c))


def eager_engine(t, rnd):
    """EagerSlidingWindowEngine.__call__ on generated volumes (smaller and larger than the window, every padding / blending mode,
    per-axis overlaps, batch sizes): the reference engine on CPU tensors against this package's engine with the gather / blend /
    finalize kernels replaced by torch stand-ins -- plan, probe window, blending order, normalisation, crop back."""
    import torch
    sys.path.insert(0, str(ROOT / "tests"))
    import test_host_lazy_tta as L
    import pytorch_connectomics_amd.inference.window as ow
    rw = S.ref("connectomics.inference.window")

    ow.ops = L._Ops

    def net(x):
        ramp = torch.linspace(0, 1, x.shape[-1]).view(1, 1, 1, 1, -1)
        return torch.cat([2 * x - 1 + ramp, 0.5 * x * x + x.mean(dim=(2, 3, 4), keepdim=True)], 1)
    cases = []
    for _ in range(120):
        roi = rnd.choice([(4, 6, 6), (6, 8, 8), (8, 8, 8), (2, 12, 10)])
        shape = tuple(rnd.choice([max(1, r - rnd.randint(0, 3)), r, r + rnd.randint(1, 9), 2 * r + rnd.randint(0, 5)]) for r in roi)
        cases.append((shape, roi, rnd.choice([0.0, 0.25, 0.5, 0.75, (0.25, 0.5, 0.5)]), rnd.choice(["constant", "bump", "gaussian", "distance_transform", "nope"]),
                      rnd.choice(["constant", "reflect", "replicate", "circular"]), rnd.choice([0.0, 0.3]), rnd.choice([1, 3, 8]), rnd.randint(0, 10 ** 6)))

    def run(mod, patch, shape, roi, overlap, mode, padding, cval, swb, seed):
        x = torch.rand((1, 1) + shape, generator=torch.Generator().manual_seed(seed))
        eng = mod.EagerSlidingWindowEngine(roi_size=roi, sw_batch_size=swb, overlap=overlap, mode=mode, padding_mode=padding, cval=cval,
                                           sw_device=None, output_device=None)
        if patch:
            eng._check_inputs = lambda inputs: torch.device("cpu")
            eng.pipeline_streams = 1
        return _tensor_digest(eng(x, net), 4)
    t.run("EagerSlidingWindowEngine (plan, probe, blending, normalisation, crop)", cases, lambda *c: run(rw, False, *c), lambda *c: run(ow, True, *c))

    bad_nets = {"mapping": lambda x: {"output": net(x)}, "list": lambda x: [net(x)], "none": lambda x: None, "rank4": lambda x: net(x)[0],
                "half": lambda x: net(x).half(), "double": lambda x: net(x).double(), "bf16": lambda x: net(x).bfloat16()}
    inputs = {"rank4": (1, 9, 9, 9), "batch2": (2, 1, 9, 9, 9), "fine": (1, 1, 9, 10, 11), "smaller_than_roi": (1, 1, 3, 5, 7), "two_channels": (1, 2, 5, 7, 9)}

    def run_bad(mod, patch, which_net, which_in):
        x = torch.rand(inputs[which_in], generator=torch.Generator().manual_seed(3))
        eng = mod.EagerSlidingWindowEngine(roi_size=(4, 6, 6), sw_batch_size=2, overlap=0.5, mode="bump", padding_mode="constant", cval=0.0,
                                           sw_device=None, output_device=None)
        if patch:
            def on_cpu(inp, _eng=eng):                       # every check of the engine but "needs a HIP device"
                try:
                    return type(_eng)._check_inputs(_eng, inp)
                except RuntimeError as e:
                    if "no CPU path" not in str(e):
                        raise
                    return torch.device("cpu")
            eng._check_inputs = on_cpu
            eng.pipeline_streams = 1
        one = lambda v: net(v[:, :1])                        # noqa: E731
        y = eng(x, bad_nets.get(which_net, one))
        return (str(y.dtype), _tensor_digest(y.float(), 3))

    def documented(case, a, b):
        """(1) accumulators are fp32 whatever the network returns and the result stays fp32 (DESIGN.md section 3 iii; the reference
        accumulates in the network's dtype): same values to the narrow type's rounding.  (2) a rank-4 network output, which the
        reference broadcasts into a (1, 2C, ...) result by accident, is refused by name."""
        if case[0] in ("half", "double", "bf16") and a[0] == b[0] == "ok":
            ra, rb = eval(a[1])[1], eval(b[1])[1]
            return ra[0] == rb[0] and all(abs(p - q) <= 2e-3 * max(1.0, abs(p)) + 0.011 for p, q in zip(ra[2:], rb[2:]))
        return case[0] == "rank4" and b[:2] == ("err", "ValueError") and "must preserve the ROI shape" in b[2]
    t.run("EagerSlidingWindowEngine: bad networks and inputs", [(n, "fine") for n in bad_nets] + [("ok", i) for i in inputs],
          lambda n, i: run_bad(rw, False, n, i), lambda n, i: run_bad(ow, True, n, i), show=12, same=documented)


def prediction_crops(t, rnd):
    rk, ok_ = S.ref("connectomics.inference.chunk_grid"), __import__("pytorch_connectomics_amd.inference.chunk_grid", fromlist=["x"])
    unit = ["1-0-0", "0-1-0", "0-0-1"]
    cases = []
    for offs in (unit, unit + ["3-0-0", "0-9-0", "0-0-27"], ["0-0-1"], ["-2-0-0", "0-3-0"], [], None):
        for mode in ("deepem", "banis", None):
            for crop in (None, [1, 1, 1], [[0, 2], [1, 1], [3, 0]], 2):
                for sel in (None, "0:3", [0], "3:"):
                    targets = [] if offs is None else [{"name": "affinity", "kwargs": {"offsets": offs, **({"affinity_mode": mode} if mode else {})}}]
                    cases.append((NS(model=NS(heads=None, primary_head=None, out_channels=len(offs or [1])),
                                     data=NS(label_transform=NS(stack_outputs=True, targets=targets)),
                                     inference=NS(model=NS(head=None, select_channel=sel, crop_pad=crop, channel_activations=None, output_dtype=None),
                                                  chunking=NS(enabled=True))),))
    t.run("resolve_global_prediction_crop", cases, rk.resolve_global_prediction_crop, ok_.resolve_global_prediction_crop)
    t.run("resolve_selected_affinity_offsets", cases, rk.resolve_selected_affinity_offsets, ok_.resolve_selected_affinity_offsets)



def small_resolvers(t, rnd):
    """The small configuration resolvers and helpers around the engines."""
    import json
    import tempfile
    import numpy as np
    import torch
    pkg = lambda name: __import__(f"pytorch_connectomics_amd.{name}", fromlist=["x"])          # noqa: E731
    rw, ow = S.ref("connectomics.inference.window"), pkg("inference.window")

    def maybe(pool):
        return rnd.choice(pool)

    def window_cfg():
        sw = NS()
        for key, pool in (("window_size", [None, [8, 8, 8], (4, 6, 8), [], [16, 16]]), ("overlap", [None, 0.5, 0.0, 1.5, -0.2, [0.25, 0.5, 0.995], (0.1, 0.2)]),
                          ("sw_batch_size", [None, 1, 4, 0, -3, "2"]), ("blending", ["bump", "constant", "gaussian", "distance", "distance_transform", "Bump", " EDT "]),
                          ("padding_mode", ["constant", "reflect", "replicate"]), ("cval", [0.0, 1, "0.5"]), ("keep_input_on_cpu", [False, True, 0, 1]),
                          ("sw_device", [None, "", "none", "cuda", "cpu", "NULL"]), ("output_device", [None, "", "None", "cpu", "cuda:0"]),
                          ("border_mask", [None, [], [2], [1, 2, 3], [1, 2], 0, ["3"]])):
            if rnd.random() < 0.7:
                setattr(sw, key, maybe(pool))
        cfg = NS()
        if rnd.random() < 0.85:
            cfg.inference = NS(sliding_window=sw) if rnd.random() < 0.9 else NS()
            if rnd.random() < 0.5:
                cfg.inference.model = NS(output_dtype=maybe([None, "float32", "fp16", "torch.bfloat16", " Half ", "float64", "int8", 16, "bf16"]))
        if rnd.random() < 0.6:
            cfg.model = NS(output_size=maybe([None, [8, 8, 8], [16, 16], (4, 4, 4), []]))
        if rnd.random() < 0.7:
            cfg.data = NS()
            if rnd.random() < 0.6:
                cfg.data.data_transform = NS(patch_size=maybe([None, [6, 6, 6], [12, 12], []]))
            if rnd.random() < 0.6:
                cfg.data.dataloader = NS(batch_size=maybe([1, 3, 0]))
            if rnd.random() < 0.5:
                cfg.data.train = NS(do_2d=maybe([True, False]))
            if rnd.random() < 0.3:
                cfg.data.val = NS(do_2d=maybe([True, False]))
        return cfg
    cfgs = [(window_cfg(),) for _ in range(600)]
    for fn in ("resolve_model_output_dtype", "is_2d_inference_mode", "resolve_inferer_roi_size"):
        t.run(f"window.{fn}", cfgs, getattr(rw, fn), getattr(ow, fn))
    t.run("window.resolve_border_mask", [(c[0], d) for c in cfgs for d in (2, 3)], rw.resolve_border_mask, ow.resolve_border_mask)
    t.run("window.resolve_inferer_overlap", cfgs, lambda c: rw.resolve_inferer_overlap(c, (8, 8, 8)), lambda c: ow.resolve_inferer_overlap(c, (8, 8, 8)))
    t.run("window._resolve_sliding_window_runtime", cfgs, lambda c: rw._resolve_sliding_window_runtime(c, (8, 8, 8)),
          lambda c: ow._resolve_sliding_window_runtime(c, (8, 8, 8)))
    t.run("window.is_distance_transform_blending", [(m,) for m in ("bump", "distance", "distance_transform", "EDT", " edt ", "constant", "dt", "Distance", "", "gaussian")],
          rw.is_distance_transform_blending, ow.is_distance_transform_blending)

    def maps(mod):
        def f(roi, mode, dt):
            v, w = mod.build_sliding_accumulator_weight_maps(roi, mode=mode, device="cpu", value_dtype=dt)
            return (_tensor_digest(v), str(v.dtype), v is w or bool(torch.equal(v, w)), tuple(w.shape))
        return f
    t.run("build_sliding_accumulator_weight_maps",
          [(tuple(rnd.randint(1, 12) for _ in range(rnd.choice((2, 3)))), m, dt) for m in ("bump", "constant", "distance", "gaussian")
           for dt in (torch.float32, torch.float16, torch.bfloat16) for _ in range(6)], maps(rw), maps(ow))

    rl, ol = S.ref("connectomics.inference.lazy"), pkg("inference.lazy")
    t.run("lazy._snap_offsets", [(rnd.randint(1, 80), rnd.randint(1, 30), rnd.randint(-2, 20), rnd.choice((0, 0, 3, 11))) for _ in range(500)],
          lambda i, r, s_, b: rl._snap_offsets(i, r, s_, border_pad=b), lambda i, r, s_, b: ol._snap_offsets(i, r, s_, border_pad=b))

    def crop_case():
        roi = tuple(rnd.randint(1, 6) for _ in range(3))
        ctx = rnd.choice([(0, 0, 0), (0, 0, 0), tuple(rnd.randint(0, 2) for _ in range(3))])
        got = tuple(r + 2 * c + rnd.choice([0, 0, 0, 1, -1]) for r, c in zip(roi, ctx))
        return (torch.arange(2 * 3 * max(1, got[0]) * max(1, got[1]) * max(1, got[2]), dtype=torch.float32).reshape(2, 3, *[max(1, g) for g in got]), roi, ctx)
    t.run("lazy._crop_prediction_to_roi", [crop_case() for _ in range(300)],
          lambda p_, r, c: _tensor_digest(rl._crop_prediction_to_roi(p_, roi_size=r, target_context=c, scope="fuzz")),
          lambda p_, r, c: _tensor_digest(ol._crop_prediction_to_roi(p_, roi_size=r, target_context=c, scope="fuzz")))

    rd, od = S.ref("connectomics.inference.lazy_distributed"), pkg("inference.lazy_distributed")

    def dist_cfg():
        cfg = NS()
        if rnd.random() < 0.9:
            cfg.inference = NS()
            if rnd.random() < 0.9:
                cfg.inference.sliding_window = NS(distributed_sharding=maybe([True, False, 1, None]))
        if rnd.random() < 0.8:
            cfg.data = NS(dataloader=NS(use_lazy_zarr=maybe([True, False]), use_lazy_h5=maybe([True, False])))
        return cfg
    t.run("lazy_distributed (single process): context, sharding switch, devices, validators, reduce", [(dist_cfg(), rnd.randint(1, 5)) for _ in range(120)],
          lambda c, n: (rd.distributed_context(), rd.is_distributed_window_sharding_enabled(c), str(rd.distributed_reduction_device(torch.device("cpu"))),
                        rd.validate_distributed_tensor_shape(torch.zeros(n), name="acc", reduction_device=torch.device("cpu")),
                        rd.validate_distributed_patch_shard(local_count=0, total_count=n, reduction_device=torch.device("cpu")),
                        rd.reduce_cpu_tensor_to_rank_zero(torch.arange(n), op=None, reduction_device=torch.device("cpu"), chunk_mb=1, name="acc").tolist()),
          lambda c, n: (od.distributed_context(), od.is_distributed_window_sharding_enabled(c), str(od.distributed_reduction_device(torch.device("cpu"))),
                        od.validate_distributed_tensor_shape(torch.zeros(n), name="acc", reduction_device=torch.device("cpu")),
                        od.validate_distributed_patch_shard(local_count=0, total_count=n, reduction_device=torch.device("cpu")),
                        od.reduce_cpu_tensor_to_rank_zero(torch.arange(n), op=None, reduction_device=torch.device("cpu"), chunk_mb=1, name="acc").tolist()))

    rc, oc = S.ref("connectomics.inference.chunked"), pkg("inference.chunked")
    rg, og = S.ref("connectomics.chunked.chunk_grid"), pkg("chunked.chunk_grid")

    def chunk_cfg():
        cfg = NS()
        if rnd.random() < 0.9:
            cfg.inference = NS()
            if rnd.random() < 0.6:
                cfg.inference.strategy = maybe(["whole_volume", "chunked", "Chunked", None, "lazy"])
            if rnd.random() < 0.8:
                ck = NS()
                for key, pool in (("enabled", [True, False, 0, 1, None]), ("shard_id", [None, 0, 1, 3, -1, "2"]), ("num_shards", [None, 1, 2, 4, 0, -2, "3"]),
                                  ("roi", [None, [4, 4, 4], [1, 2, 3, 7, 8, 9], [1, 2], [3, 3, 3, 3, 9, 9], [0, 0, 0], (5, 6, 7), ["4", "4", "4"]])):
                    if rnd.random() < 0.7:
                        setattr(ck, key, maybe(pool))
                cfg.inference.chunking = ck
        return cfg
    ccfgs = [(chunk_cfg(),) for _ in range(500)]
    for fn in ("is_chunked_inference_enabled", "_resolve_external_chunk_shard", "is_external_chunk_sharding_enabled", "_resolve_inference_roi"):
        t.run(f"chunked.{fn}", ccfgs, getattr(rc, fn), getattr(oc, fn))

    def roi_cases():
        for _ in range(300):
            vol = tuple(rnd.randint(4, 60) for _ in range(3))
            chunk = tuple(rnd.randint(2, 25) for _ in range(3))
            crop = tuple(rnd.randint(0, 4) for _ in range(3))
            lo = tuple(rnd.randint(0, v) for v in vol)
            hi = tuple(l + rnd.randint(1, 40) for l in lo)
            yield vol, chunk, crop, lo, hi
    t.run("chunked._filter_chunks_to_roi", list(roi_cases()),
          lambda v, c, cr, lo, hi: rc._filter_chunks_to_roi(rg.build_chunk_grid(v, c), (lo, hi), cr),
          lambda v, c, cr, lo, hi: oc._filter_chunks_to_roi(og.build_chunk_grid(v, c), (lo, hi), cr))

    def abiss(mod):
        def f(shape, seed):
            a = np.random.default_rng(seed).random(shape, dtype=np.float32)
            out = mod._to_abiss_affinity_convention(a)
            return (out.shape, str(out.dtype), float(np.abs(out).sum()), out.reshape(-1)[:: max(1, out.size // 17)].tolist())
        return f
    t.run("chunked._to_abiss_affinity_convention", [((c, rnd.randint(1, 6), rnd.randint(1, 6), rnd.randint(1, 6)), i) for i, c in enumerate([3] * 40 + [1, 2, 4, 6])],
          abiss(rc), abiss(oc))

    rm, om = S.ref("connectomics.chunked.manifest"), pkg("chunked.manifest")

    def manifest_script(mod):
        def f(cfg_a, cfg_b, keys, overwrite):
            with tempfile.TemporaryDirectory() as d:
                path = Path(d) / "resume.json"
                m = mod.ResumeManifest.load_or_create(path, cfg_a)
                m.mark_completed(keys[0]); m.mark_completed(keys[0]); m.mark_many(keys)
                first = json.loads(path.read_text())
                m2 = mod.ResumeManifest.load_or_create(path, cfg_b, overwrite=overwrite)
                m2.mark_many(keys[:1])
                return (first, sorted(m2.completed), json.loads(path.read_text()), sorted(p.name for p in Path(d).iterdir()))
        return f

    def manifest_cases():
        base = {"chunk_shape": [8, 8, 8], "overlap": 0.5, "output_dtype": "float32", "output_shape": [16, 16, 16], "note": "a"}
        for _ in range(120):
            other = dict(base)
            for k in list(other):
                r = rnd.random()
                if r < 0.15:
                    other.pop(k)
                elif r < 0.35:
                    other[k] = {"chunk_shape": [4, 8, 8], "overlap": 0.25, "output_dtype": "uint8", "output_shape": [16, 16, 8], "note": "b"}[k]
            keys = [f"z{rnd.randint(0, 3)}_y{rnd.randint(0, 3)}_x0" for _ in range(rnd.randint(1, 5))]
            yield base, other, keys, rnd.random() < 0.3
    t.run("ResumeManifest (create, mark, reload, mismatch, overwrite)", list(manifest_cases()), manifest_script(rm), manifest_script(om),
          same=lambda case, a, b: a[0] == b[0] == "err" and a[1] == b[1] and a[2].split("resume.json")[-1] == b[2].split("resume.json")[-1])

    ru, ou = S.ref("connectomics.utils.model_outputs"), pkg("utils.model_outputs")

    def head_cfg():
        cfg = NS()
        heads = maybe([None, {}, {"aff": NS(out_channels=3, target_slice="0:3")}, {"aff": NS(out_channels=3), "sdt": NS(out_channels=1, target_slice=[3])},
                       {"a": {"out_channels": 2, "target_slice": "0:2"}, "b": {"out_channels": 1}, "c": {"out_channels": 4}}])
        cfg.model = NS(out_channels=maybe([1, 3, None]))
        if heads is not None:
            cfg.model.heads = heads
        if rnd.random() < 0.5:
            cfg.model.primary_head = maybe([None, "aff", "sdt", "a", "zz", "", 3])
        if rnd.random() < 0.8:
            cfg.inference = NS(model=NS())
            if rnd.random() < 0.6:
                cfg.inference.model.head = maybe([None, "aff", "sdt", "a,b", "a, c ,b", "b,zz", ",", "", " aff ", "c", 5])
            if rnd.random() < 0.5:
                cfg.inference.model.select_channel = maybe([None, [0, 1], "0:2", -1])
            if rnd.random() < 0.5:
                cfg.inference.model.channel_activations = maybe([None, [], [["0:3", "sigmoid"]], ({"channels": "0", "activation": "tanh"},), "sigmoid"])
        return cfg
    hcfgs = [head_cfg() for _ in range(500)]
    reqs = [None, "aff", "sdt", "a", "a,b", "zz", "", "  ", 3, "b, c", "a,zz"]
    for fn in ("get_inference_model_config", "get_inference_select_channel", "get_inference_channel_activations", "get_model_head_names", "get_total_model_head_channels",
               "resolve_output_heads", "resolve_configured_output_head", "resolve_configured_output_channels"):
        t.run(f"model_outputs.{fn}", [(c,) for c in hcfgs], lambda c, fn=fn: _plain_ns(getattr(ru, fn)(c)), lambda c, fn=fn: _plain_ns(getattr(ou, fn)(c)))
    t.run("model_outputs.resolve_output_head", [(c, rnd.choice(reqs), rnd.random() < 0.5) for c in hcfgs],
          lambda c, r, an: ru.resolve_output_head(c, requested_head=r, purpose="fuzz", allow_none=an),
          lambda c, r, an: ou.resolve_output_head(c, requested_head=r, purpose="fuzz", allow_none=an))
    t.run("model_outputs.resolve_output_channels", [(c, rnd.choice(reqs), rnd.random() < 0.5) for c in hcfgs],
          lambda c, r, aa: ru.resolve_output_channels(c, requested_head=r, purpose="fuzz", allow_ambiguous=aa),
          lambda c, r, aa: ou.resolve_output_channels(c, requested_head=r, purpose="fuzz", allow_ambiguous=aa))
    t.run("model_outputs.resolve_head_target_slice", [(c, rnd.choice(["aff", "sdt", "a", "b", "zz"])) for c in hcfgs], ru.resolve_head_target_slice, ou.resolve_head_target_slice)

    def outputs():
        x, y = torch.zeros(1, 2, 2), torch.ones(1, 3, 3)
        return maybe([x, {"output": x}, {"output": x, "ds_1": y}, {"output": {"a": x, "b": y}}, {"a": x}, {"output": {}}, {"output": {"a": x}}, {"output": {"a": 5}},
                      [x], None, {"output": None}, {"b": y, "a": x}])

    def select(mod):
        def f(out, req, primary):
            tns, head = mod.select_output_tensor(out, requested_head=req, primary_head=primary, purpose="fuzz")
            return (tuple(tns.shape), head)
        return f
    t.run("model_outputs.select_output_tensor", [(outputs(), rnd.choice([None, "a", "b", "zz"]), rnd.choice([None, "a", "b", "zz"])) for _ in range(400)],
          select(ru), select(ou))

    rr, orr = S.ref("connectomics.models.architectures.registry"), pkg("models.architectures.registry")

    def registry_script(mod):
        def f(ops):
            import warnings
            saved = dict(mod._ARCHITECTURE_REGISTRY)
            mod._ARCHITECTURE_REGISTRY.clear()
            log = []
            try:
                for op, name in ops:
                    with warnings.catch_warnings(record=True) as caught:
                        warnings.simplefilter("always")
                        try:
                            if op == "register":
                                def builder(cfg, _n=name):
                                    """doc of the builder."""
                                    return _n
                                mod.register_architecture(name)(builder)
                                log.append(("registered", name))
                            elif op == "get":
                                log.append(("built", mod.get_architecture_builder(name)(None)))
                            elif op == "has":
                                log.append(("has", mod.is_architecture_available(name)))
                            elif op == "drop":
                                log.append(("dropped", mod.unregister_architecture(name)))
                            elif op == "list":
                                log.append(("list", mod.list_architectures()))
                            else:
                                log.append(("info", {k: sorted(v) for k, v in mod.get_architecture_info().items()}))
                        except Exception as e:      # noqa: BLE001
                            log.append(("err", type(e).__name__, str(e)))
                        log.append(("warnings", [str(w.message) for w in caught]))
                return log
            finally:
                mod._ARCHITECTURE_REGISTRY.clear()
                mod._ARCHITECTURE_REGISTRY.update(saved)
        return f
    names = ["unet", "mednext", "rsunet", "x"]
    t.run("architecture registry (register / overwrite / get / has / drop / list / info)",
          [([(rnd.choice(["register", "register", "get", "has", "drop", "list", "info"]), rnd.choice(names)) for _ in range(rnd.randint(3, 12))],) for _ in range(200)],
          registry_script(rr), registry_script(orr))


def _plain_ns(v):
    if isinstance(v, NS):
        return {k: _plain_ns(x) for k, x in sorted(vars(v).items())}
    if isinstance(v, dict):
        return {k: _plain_ns(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain_ns(x) for x in v]
    return v


def patch_first_local(t, rnd):
    """Patch-first-local TTA (the reference default; tta.py:880-1314) through REAL sliding engines on both sides: the reference predictor +
    its engine on CPU tensors against this package's predictor + engine with the device kernels replaced by the torch stand-ins
    (view-coded gather / blend, affinity channel maps, per-shift weights: tests/test_host_lazy_tta.py `_Ops`).  Plain and
    directional-affinity outputs; flips and quarter turns; blending modes, overlaps, ensemble modes, channel selection, masks."""
    import torch
    sys.path.insert(0, str(ROOT / "tests"))
    import test_host_lazy_tta as L
    import pytorch_connectomics_amd.inference.tta as otta
    import pytorch_connectomics_amd.inference.tta_ensemble as oens
    import pytorch_connectomics_amd.inference.window as ow
    rtta, rw = S.ref("connectomics.inference.tta"), S.ref("connectomics.inference.window")
    otta.ops = oens.ops = ow.ops = L._Ops

    def net3(x):
        z = torch.linspace(-1, 1, x.shape[2]).view(1, 1, -1, 1, 1)
        y = torch.linspace(-1, 1, x.shape[3]).view(1, 1, 1, -1, 1)
        w = torch.linspace(-1, 1, x.shape[4]).view(1, 1, 1, 1, -1)
        return torch.cat([x * (1.0 + 0.5 * w) + 0.25 * y, torch.tanh(2 * x - 1) * z + 0.1 * w * y, 3 * x * x - 1.5 * w + z * y], 1)

    def anet(n):
        def f(x):
            parts = net3(x)
            return torch.cat([parts, 0.5 * parts + 0.1], 1)[:, :n]
        return f

    def cfg_of(kw):
        offs = kw.get("offsets")
        return NS(model=NS(primary_head=None, heads=None, out_channels=len(offs) if offs else 3),
                  data=NS(train=NS(do_2d=False), val=NS(do_2d=False), dataloader=NS(batch_size=1),
                          label_transform=None if not offs else NS(stack_outputs=True, targets=[
                              {"name": "affinity", "kwargs": {"offsets": offs, "affinity_mode": kw["amode"]}}])),
                  inference=NS(sliding_window=NS(window_size=list(kw["roi"]), sw_batch_size=kw["swb"], overlap=kw["overlap"], blending=kw["blending"],
                                                 padding_mode="constant", cval=0.0, keep_input_on_cpu=False, sw_device=None, output_device=None,
                                                 border_mask=[], distributed_sharding=False),
                               model=NS(head=None, select_channel=kw["select"], output_dtype=None, channel_activations=kw["acts"], crop_pad=None),
                               test_time_augmentation=NS(enabled=True, flip_axes=kw["flips"], rotation90_axes=kw["rot"], rotate90_k=kw["ks"],
                                                         ensemble_mode=kw["mode"], patch_first_local=kw["patch_first"], distributed_sharding=False,
                                                         apply_mask=True, empty_cache_interval=0)))
    unit = ["1-0-0", "0-1-0", "0-0-1"]
    cases = []
    for _ in range(140):
        square = rnd.random() < 0.6
        roi = rnd.choice([(4, 6, 6), (5, 8, 8), (6, 6, 6)]) if square else rnd.choice([(4, 6, 8), (5, 7, 6)])
        shape = tuple(r + rnd.choice([0, 2, 5, r]) for r in roi)
        if square:
            shape = (shape[0], shape[1], shape[1])
        rot = rnd.choice([None, [[1, 2]]]) if square else None
        affinity = rnd.random() < 0.5
        offs = rnd.choice([unit, unit + ["2-0-0", "0-3-0", "0-0-3"], unit + ["3-0-0", "0-2-0", "0-0-2"]]) if affinity else None
        cases.append(dict(roi=roi, shape=shape, swb=rnd.choice([1, 2, 4]), overlap=rnd.choice([0.0, 0.25, 0.5, (0.25, 0.5, 0.5)]),
                          blending=rnd.choice(["constant", "bump", "bump", "distance_transform"]), flips=rnd.choice(["all", [[0]], [[1, 2]], [[2], [0, 1]], None]), rot=rot,
                          ks=rnd.choice([None, [1], [1, 3], [0, 2]]) if rot else None, mode=rnd.choice(["mean", "min", "max", [["0", "max"], ["1:", "mean"]]]),
                          select=rnd.choice([None, [2, 0], "0:2", [1]]),
                          acts=rnd.choice([None, [{"channels": ":", "activation": "sigmoid"}], [{"channels": "0", "activation": "tanh"}]]),
                          offsets=offs, amode=rnd.choice(["deepem", "banis"]), patch_first=rnd.random() < 0.8, use_mask=rnd.random() < 0.3,
                          seed=rnd.randint(0, 10 ** 6)))

    def run(tta_mod, win_mod, patch, kw):
        cfg = cfg_of(kw)
        g = torch.Generator().manual_seed(kw["seed"])
        x = torch.rand((1, 1) + kw["shape"], generator=g)
        mask = (torch.rand((1, 1) + kw["shape"], generator=g) > 0.4).float() if kw["use_mask"] else None
        eng = win_mod.build_sliding_inferer(cfg)
        if patch:
            eng._check_inputs = lambda inp: torch.device("cpu")
            eng.pipeline_streams = 1
        network = anet(len(kw["offsets"])) if kw["offsets"] else net3
        p = tta_mod.TTAPredictor(cfg=cfg, sliding_inferer=eng, forward_fn=network)
        return _tensor_digest(p.predict(x, mask=mask), 3)

    def close(case, a, b):
        """fp32 summation order inside a window batch differs by construction (one scatter per window in order here, the reference adds
        whole patches): equal to rounding."""
        if a[0] != "ok" or b[0] != "ok":
            return False
        ra, rb = eval(a[1]), eval(b[1])
        return ra[:2] == rb[:2] and all(abs(u - v) <= 2e-3 * max(1.0, abs(u)) for u, v in zip(ra[2:], rb[2:]))
    t.run("TTAPredictor.predict through sliding engines (patch-first-local and whole-volume views, plain and affinity outputs)",
          [(kw,) for kw in cases], lambda kw: run(rtta, rw, False, kw), lambda kw: run(otta, ow, True, kw), same=close, show=6)


if __name__ == "__main__":
    sys.exit(1 if main() else 0)

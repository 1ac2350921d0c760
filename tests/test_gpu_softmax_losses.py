"""GPU checks of the softmax-loss kernels (csrc/softmax_loss_kernels.hip) and of the losses finalised from their sums.

Sweep: six shapes (odd sizes, one voxel row of 131, C = 5 and C = 32 across two and four lanes, a 2-D input, and eighteen tiles with a
ragged tail) x three layouts (channels-last, contiguous NCDHW, channels 1 : 1 + C of a channels-last tensor with C + 3 channels) x
three target kinds x (no mask, a one-channel mask, a C-channel mask).

Exact plumbing.  Logits are +20 at class k_v and -20 elsewhere, labels y_v come from a second map.  In fp32 exp(-40) vanishes against
1, so the softmax sum is exactly 1, lse exactly 20, -logp exactly 0 or 40 and p exactly 1 or exp(-40) = 4.2e-18.  Columns 3, 4, 5, 7
are then integers (column 5 = 40 x a count; column 6 = 40 x the voxels predicted as another class, 40 (C - 1) #CE-valid over the
classes) that the CPU forms from the two index maps alone; they are held exactly (below 2^24 every partial sum is exact in any
order); the index targets carry ignore_index at a tenth of their voxels, which leave columns 0, 3, 4, 5, 7 (t = 0) and column 6
(valid = 0).  Column 0 is its count exactly wherever the count is not 0; a class that is never hit keeps its mismatches' exp(-40) each
(1.3e-17 for three of them), so there the bound is 4.3e-18 x #mismatches.  Columns 1 and 2 may differ from their counts by 1e-9 R.  At a
masked voxel every logit reads -20, so p = 1 / C and -logp = log C there, which are not integers: with a mask columns 3, 4 and 7 stay
exact and columns 0, 1, 2, 5, 6 are held to 1e-6 of the fp64 sums of the same voxel-by-voxel model (the floor of this suite: fp32
rounding of log C and 1 / C, 6e-8 each, and of a few hundred additions).

Against fp64.  For random logits (sigma 4, some beyond the clamp) every loss, value and gradient, is held to 4 x the error of the fp32
torch restatement on the CPU against the fp64 restatement, plus 1e-6: the value relatively, the gradient as relative L2 and as
max |err| / max |g|.  No voxel is excluded.
"""
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import softmax_loss_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).parent / "golden"
FACTOR, FLOOR = 4.0, 1e-6
GUARD = 64
BAD_OPS = ("aten::_softmax", "aten::_log_softmax", "aten::nll_loss", "aten::one_hot", "aten::masked_fill")
SWEEP = [(s, l, t, m) for s in SC.GPU_SHAPES for l in SC.LAYOUTS for t in SC.TARGET_KINDS for m in SC.MASK_KINDS]


def _sweep_id(c):
    return f"{SC.shape_id(c[0])}-{c[1]}-{c[2]}-{c[3]}"


def _sl():
    from pytorch_connectomics_amd.training import softmax_loss_autograd as sl
    return sl


def _ops():
    from pytorch_connectomics_amd import hip_ops as ops
    return ops


def _operands(shape, layout, target_kind, mask_kind, exact, clamp=False):
    """-> (the CPU case, logits on the device in `layout`, their allocation, target, mask); `clamp`: the logits the module hands its
    losses, clamped to +-20 (on the CPU tensors too)"""
    made = (SC.gpu_exact_case if exact else SC.gpu_random_case)(shape, target_kind, mask_kind)
    if clamp:
        made = (torch.clamp(made[0], -20.0, 20.0),) + tuple(made[1:])
    logits, target, mask = made[:3]
    x, store = SC.to_layout(logits, layout, "cuda")
    t = SC.to_layout(target, "channels_last" if layout != "contiguous" else "contiguous", "cuda")[0] if target_kind == "dense" \
        else target.cuda()
    m = None
    if mask is not None:
        m = SC.to_layout(mask, "channels_last" if layout != "contiguous" and mask_kind == "full" else "contiguous", "cuda")[0]
    return made, x, store, t, m


def test_tile_size_is_the_librarys():
    from pytorch_connectomics_amd import _native as nat
    lib = nat.lib()
    assert lib.pytc_softmax_loss_tiles(SC.TILE) == 1 and lib.pytc_softmax_loss_tiles(SC.TILE + 1) == 2 and lib.pytc_softmax_loss_tiles(1) == 1
    R = int(np.prod(SC.GPU_SHAPES[-1][2:]))
    assert lib.pytc_softmax_loss_tiles(R) >= 4 and R % SC.TILE != 0                # three full tiles at least, and a ragged tail


# ---- exact plumbing ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SWEEP, ids=_sweep_id)
def test_sums_of_one_hot_logits_are_the_integer_counts(case):
    shape, layout, target_kind, mask_kind = case
    (logits, target, mask, k, y), x, _, t, m = _operands(shape, layout, target_kind, mask_kind, exact=True)
    N, C = shape[:2]
    R = int(np.prod(shape[2:]))
    S = _ops().softmax_loss_forward(x, t, m, ignore_index=-100, fill=-20.0).cpu().double()
    assert S.shape == (N, C, 8)
    # what every (sample, class, voxel) element reads, from the maps alone
    kk = torch.zeros(shape, dtype=torch.float64).scatter_(1, k.unsqueeze(1), 1.0)             # 1 where the logit is +20
    ign = (y == -100).unsqueeze(1)                                                            # index kinds only: t = 0, CE-invalid
    tt = torch.zeros(shape, dtype=torch.float64).scatter_(1, y.clamp_min(0).unsqueeze(1), 1.0) * (~ign)
    assert target_kind == "dense" or int(ign.sum()) > 0 or ign.numel() < 40
    if mask is None:
        live = torch.ones(shape, dtype=torch.bool)
    else:
        live = (mask > 0).expand(shape)
    full = live.all(1, keepdim=True)                                                          # the voxel has no masked channel
    if target_kind == "dense":
        tt = tt * live
    else:
        zero = torch.zeros(shape, dtype=torch.float64)
        zero[:, 0] = 1.0
        tt = torch.where(full, tt, zero)                                                      # the label reads 0 ...
        ign = ign & full                                                                      # ... and is then not ignored
    valid = (~ign).double()
    sums = lambda a: a.flatten(2).sum(-1)                                                     # noqa: E731
    assert torch.equal(S[..., 3], sums(tt)) and torch.equal(S[..., 4], sums(tt)) and torch.equal(S[..., 7], sums(tt)), "t columns"
    if mask is None:
        # column 0 = #hits + #mismatches x exp(-40): the second part (at most 4.3e-18 R) vanishes in fp32 against any hit, and is all
        # there is for a class without one (C = 32 on 105 voxels), so: the count exactly after rounding, and no further than that part
        hits = sums(kk * tt)
        assert torch.equal(S[..., 0].round(), hits) and bool(((S[..., 0] - hits).abs() <= 4.3e-18 * sums((1.0 - kk) * tt)).all()), \
            "column 0: voxels where the prediction hits the label"
        assert torch.equal(S[..., 0][hits > 0], hits[hits > 0])
        assert torch.equal(S[..., 5], 40.0 * sums((1.0 - kk) * tt)), "column 5: 40 x mismatches"
        assert torch.equal(S[..., 6], 40.0 * sums(valid * (1.0 - kk))), "column 6: 40 x the CE-valid voxels predicted as another class"
        assert float((S[..., 1] - sums(kk)).abs().max()) <= 1e-9 * R and float((S[..., 2] - sums(kk)).abs().max()) <= 1e-9 * R
        return
    # with a mask: the softmax of (logit or -20) in fp64, voxel by voxel
    xm = torch.where(live, logits.double(), torch.full((), -20.0, dtype=torch.float64))
    logp = torch.log_softmax(xm, 1)
    p = logp.exp()
    for col, want in ((0, p * tt), (1, p), (2, p * p), (5, -tt * logp), (6, -valid * logp)):
        w = sums(want)
        assert float(((S[..., col] - w).abs() / w.abs().clamp_min(1.0)).max()) <= 1e-6, col


# ---- spatially sliced operands -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", ["last_dim_kept_one", "middle_dim_kept_one", "every_other_plane"])
def test_spatially_sliced_logits_read_their_own_voxels(cut):
    """a size-1 spatial dim says nothing about the addresses: [..., 0:1] collapses with the row stride of the wider tensor,
    [:, :, :, 0:1, :] and [:, :, ::2] do not collapse and are copied; sums and dx equal those of the contiguous copy, bit for bit"""
    g = torch.Generator().manual_seed(21)
    wide = (torch.randn(2, 3, 4, 5, 6, generator=g) * 4).cuda()
    x = {"last_dim_kept_one": wide[..., 0:1], "middle_dim_kept_one": wide[:, :, :, 0:1, :], "every_other_plane": wide[:, :, ::2]}[cut]
    assert not x.is_contiguous()
    y = torch.randint(0, 3, x.shape[:1] + x.shape[2:], generator=g).cuda()
    gs = torch.randn(2, 3, 8, generator=g).cuda()
    ops = _ops()
    xc = x.contiguous()
    assert torch.equal(ops.softmax_loss_forward(x, y), ops.softmax_loss_forward(xc, y))
    dx = ops.softmax_loss_backward(gs, x, y)
    assert dx.shape == x.shape and torch.equal(dx, ops.softmax_loss_backward(gs, xc, y))
    want = _sl().softmax_loss_sums_torch(x.cpu().double(), y.cpu())
    assert torch.allclose(ops.softmax_loss_forward(x, y).cpu().double(), want, rtol=1e-5, atol=1e-6)


# ---- against fp64 --------------------------------------------------------------------------------------------------------------------------
def _losses_for(target_kind):
    onehot = target_kind != "dense"
    sl = _sl()
    out = {
        "CrossEntropyLoss": (sl.cross_entropy_loss, {}),
        "CrossEntropyLoss-weighted-smoothed": (sl.cross_entropy_loss, {"label_smoothing": 0.1, "weight": "ramp"}),
        "CrossEntropyLoss-sum": (sl.cross_entropy_loss, {"reduction": "sum"}),
        "DiceLoss": (sl.softmax_dice_loss, {"softmax": True, "to_onehot_y": onehot}),
        "DiceLoss-squared-nobg": (sl.softmax_dice_loss, {"softmax": True, "to_onehot_y": onehot, "squared_pred": True,
                                                         "include_background": False}),
        "DiceCELoss": (sl.dice_ce_loss, {"softmax": True, "to_onehot_y": onehot, "lambda_ce": 0.5}),
        "GeneralizedDiceLoss": (sl.generalized_dice_loss, {"softmax": True, "to_onehot_y": onehot}),
        "GeneralizedDiceLoss-simple": (sl.generalized_dice_loss, {"softmax": True, "to_onehot_y": onehot, "w_type": "simple"}),
    }
    return out


def _eval(fn, kw, x, t, m, C):
    kw = dict(kw)
    if kw.get("weight") == "ramp":
        kw["weight"] = [0.5 + 0.25 * c for c in range(C)]
    x = x.detach().requires_grad_(True)
    v = fn(x, t, m, fill=-20.0, **kw)
    (g,) = torch.autograd.grad(v, x)
    return v, g


def _check_against_fp64(what, hip, f32, f64):
    def rel(a, r):
        return abs(a - r) / max(abs(r), 1e-300)
    ek, er = rel(hip[0], f64[0]), rel(f32[0], f64[0])
    scale = f64[1].abs().max().clamp_min(1e-300)
    nrm = f64[1].norm().clamp_min(1e-300)
    lk, lr = float((hip[1] - f64[1]).norm() / nrm), float((f32[1] - f64[1]).norm() / nrm)
    mk, mr = float((hip[1] - f64[1]).abs().max() / scale), float((f32[1] - f64[1]).abs().max() / scale)
    print(f"{what}: value {hip[0]:.9g} (fp64 {f64[0]:.12g}) rel err {ek:.3g}, restatement {er:.3g}, bound {FACTOR * er + FLOOR:.3g}; "
          f"grad rel L2 {lk:.3g}, restatement {lr:.3g}, bound {FACTOR * lr + FLOOR:.3g}; max |err| / max |g| {mk:.3g}, restatement "
          f"{mr:.3g}, bound {FACTOR * mr + FLOOR:.3g}")
    return ek <= FACTOR * er + FLOOR and lk <= FACTOR * lr + FLOOR and mk <= FACTOR * mr + FLOOR


@pytest.mark.parametrize("layout", SC.LAYOUTS)
@pytest.mark.parametrize("shape", SC.GPU_SHAPES, ids=SC.shape_id)
def test_losses_are_within_four_times_the_fp32_restatement_error(shape, layout):
    """every target kind x mask kind x loss of one (shape, layout); two runs of the kernels give the same bits"""
    failed = []
    C = shape[1]
    for target_kind in SC.TARGET_KINDS:
        for mask_kind in SC.MASK_KINDS:
            (xc, target, mask), x, _, t, m = _operands(shape, layout, target_kind, mask_kind, exact=False, clamp=True)
            assert float(xc.abs().max()) == 20.0                       # some logits lay beyond the clamp
            for name, (fn, kw) in _losses_for(target_kind).items():
                v, g = _eval(fn, kw, x, t, m, C)
                assert v.is_cuda and v.dtype == torch.float32 and g.dtype == torch.float32 and g.shape == x.shape
                v2, g2 = _eval(fn, kw, x, t, m, C)
                assert torch.equal(v, v2) and torch.equal(g, g2), "not bit-reproducible"
                res = {}
                for dt in (torch.float32, torch.float64):
                    tc = target if target.dtype == torch.int64 else target.to(dt)
                    vc, gc = _eval(fn, kw, xc.to(dt), tc, None if mask is None else mask.to(dt), C)
                    res[dt] = (float(vc.detach().double()), gc.double())
                what = f"{SC.shape_id(shape)} {layout} {target_kind} mask={mask_kind} {name}"
                if not _check_against_fp64(what, (float(v.double().cpu()), g.double().cpu()), res[torch.float32], res[torch.float64]):
                    failed.append(what)
    assert not failed, failed


# ---- the reference fixtures on the kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.CE_CASES))
def test_cross_entropy_fixtures_on_the_device(name):
    gold = np.load(GOLD / "softmax_losses.npz")
    logits, target = torch.from_numpy(gold[f"{name}__logits"]), torch.from_numpy(gold[f"{name}__target"])
    kw = SC.ce_kwargs(name)
    kw_dev = {k: (v.tolist() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    sl = _sl()
    x = logits.cuda().requires_grad_(True)
    v = sl.cross_entropy_loss(x, target.cuda(), **kw_dev)
    (g,) = torch.autograd.grad(v, x)
    x64 = logits.double().requires_grad_(True)
    v64 = sl.cross_entropy_loss(x64, target, **kw_dev)
    (g64,) = torch.autograd.grad(v64, x64)
    ref = (float(gold[f"{name}__loss"]), torch.from_numpy(gold[f"{name}__grad"]).double())
    assert _check_against_fp64(name, (float(v.double().cpu()), g.double().cpu()), ref, (float(v64.detach()), g64)), name


@pytest.mark.parametrize("which", ["ds", "plain"])
def test_orchestrator_fixtures_on_the_device(which):
    from pytorch_connectomics_amd.training.module import ConnectomicsModule
    gold = np.load(GOLD / "softmax_losses.npz")
    pre = f"orch_{which}__"
    names = [k[len(pre) + 3:] for k in gold.files if k.startswith(pre + "in_")]
    m = ConnectomicsModule(SC.orch_cfg(which == "ds"), model=torch.nn.Identity())

    def run(conv):
        outs = {k: conv(torch.from_numpy(gold[f"{pre}in_{k}"])).requires_grad_(True) for k in names}
        total, _ = m._compute_loss(outs if which == "ds" else outs["output"], conv(torch.from_numpy(gold[pre + "labels"])),
                                   conv(torch.from_numpy(gold[pre + "mask"])))
        grads = torch.autograd.grad(total, [outs[k] for k in names])
        return float(total.detach().double().cpu()), torch.cat([g.detach().double().cpu().flatten() for g in grads])

    ref = (float(gold[pre + "total"]), torch.cat([torch.from_numpy(gold[f"{pre}grad_{k}"]).double().flatten() for k in names]))
    assert _check_against_fp64(f"orchestrator {which}", run(lambda t: t.cuda()), ref, run(lambda t: t.double()))


# ---- guarded buffers -----------------------------------------------------------------------------------------------------------------------
def _guarded(n, dtype=torch.float32):
    fill = float("nan") if dtype.is_floating_point else -(2 ** 40)
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf[GUARD:GUARD + n], buf


def _guarded_copy(t):
    """the tensor's MEMORY (its storage extent, whatever its strides) between guard words -> a view of the same shape and strides"""
    t = t.cuda()
    if t.dim() >= 3 and not t.is_contiguous():
        raise AssertionError("pass contiguous tensors or use _guarded_layout")
    flat, buf = _guarded(t.numel(), t.dtype)
    flat.copy_(t.reshape(-1))
    return flat.view(t.shape), buf


def _guarded_layout(x, layout, sentinel):
    """x in `layout` inside a guarded allocation; the sliced layout's other channels hold the sentinel"""
    view, store = SC.to_layout(x, layout, "cuda", sentinel=sentinel)
    flat, buf = _guarded(store.numel(), store.dtype)
    flat.copy_(store.reshape(-1))
    inner = flat.view(store.shape)
    if layout == "contiguous":
        return inner, buf, inner
    inv = (0, x.dim() - 1) + tuple(range(1, x.dim() - 1))
    v = inner.permute(inv)
    return (v if layout == "channels_last" else v[:, 1:1 + x.shape[1]]), buf, inner


def _guards_intact(buf, what):
    if buf.dtype.is_floating_point:
        assert bool(buf[:GUARD].isnan().all()) and bool(buf[-GUARD:].isnan().all()), f"{what}: a guard word was written"
    else:
        assert bool((buf[:GUARD] == -(2 ** 40)).all()) and bool((buf[-GUARD:] == -(2 ** 40)).all()), f"{what}: a guard word was written"


@pytest.mark.parametrize("case", [c for c in SWEEP if c[3] != "one" or c[1] == "sliced"], ids=_sweep_id)
def test_guarded_buffers_stay_intact_and_every_output_has_a_writer(case):
    from pytorch_connectomics_amd import _native as nat
    shape, layout, target_kind, mask_kind = case
    logits, target, mask = SC.gpu_random_case(shape, target_kind, mask_kind)
    N, C = shape[:2]
    R = int(np.prod(shape[2:]))
    SENT = 12345.0
    x, xbuf, _ = _guarded_layout(logits, layout, SENT)
    bufs = {"x": xbuf}
    if target_kind == "dense":
        t, bufs["target"], _ = _guarded_layout(target, "contiguous" if layout == "contiguous" else "channels_last", SENT)
    else:
        t, bufs["target"] = _guarded_copy(target)
    m = None
    if mask is not None:
        m, bufs["mask"] = _guarded_copy(mask)
    part, bufs["partial"] = _guarded(8 * N * C * nat.lib().pytc_softmax_loss_tiles(R))
    sums_flat, bufs["sums"] = _guarded(N * C * 8)
    sums = sums_flat.view(N, C, 8)
    dx, bufs["dx"], dstore = _guarded_layout(torch.full(shape, float("inf")), layout, SENT)
    ops = _ops()
    got = ops.softmax_loss_forward(x, t, m, _buffers=(part, sums))
    gs = torch.randn(N, C, 8, generator=torch.Generator().manual_seed(1)).cuda()
    ops.softmax_loss_backward(gs, x, t, m, out=dx)
    torch.cuda.synchronize()
    for name, buf in bufs.items():
        _guards_intact(buf, f"{_sweep_id(case)} {name}")
    assert got.data_ptr() == sums.data_ptr() and not bool(part.isnan().any()) and not bool(sums.isnan().any()), "partial / sums: no writer"
    assert bool(torch.isfinite(dx).all()), "dx: an element has no writer"
    if layout == "sliced":
        assert bool((dstore[..., 0] == SENT).all()) and bool((dstore[..., 1 + C:] == SENT).all()), "dx: a gap between the slices was written"
    # and the guarded call computes what the plain call does, bit for bit
    assert torch.equal(sums, ops.softmax_loss_forward(x, t, m))
    assert torch.equal(dx, ops.softmax_loss_backward(gs, x, t, m))


# ---- masking and ignoring ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", SC.LAYOUTS)
@pytest.mark.parametrize("shape", [SC.GPU_SHAPES[0], SC.GPU_SHAPES[2], SC.GPU_SHAPES[4]], ids=SC.shape_id)
def test_masked_and_ignored_voxels_get_exact_zeros(shape, layout):
    ops = _ops()
    N, C = shape[:2]
    for mask_kind in ("one", "full"):
        (logits, target, mask), x, _, t, m = _operands(shape, layout, "index_long", mask_kind, exact=False)
        gs = torch.randn(N, C, 8, generator=torch.Generator().manual_seed(2)).cuda()
        dx = ops.softmax_loss_backward(gs, x, t, m).cpu()
        dead = ~(mask > 0).expand(shape)
        assert int(dead.sum()) > 0 and bool((dx[dead] == 0).all()), "dx at masked elements"
        assert float(dx[~dead].abs().max()) > 0
    # the CE part alone (only columns 5 and 6 carry a gradient): exactly 0 at ignored voxels
    (logits, target, _), x, _, t, _ = _operands(shape, layout, "index_long", "none", exact=False)
    gs = torch.zeros(N, C, 8)
    gs[..., 5:7] = torch.randn(N, C, 2, generator=torch.Generator().manual_seed(3))
    dx = ops.softmax_loss_backward(gs.cuda(), x, t, None).cpu()
    ignored = (target == -100).unsqueeze(1).expand(shape)
    assert int(ignored.sum()) > 0 and bool((dx[ignored] == 0).all()) and float(dx[~ignored].abs().max()) > 0


# ---- an out-of-range label -----------------------------------------------------------------------------------------------------------------
def test_out_of_range_label_gives_nan_and_no_device_error():
    from pytorch_connectomics_amd.training.module import ConnectomicsModule
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, 4, 6, 7, generator=g).cuda()
    y = torch.randint(0, 3, (2, 1, 4, 6, 7), generator=g).float()
    y[1, 0, 2, 3, 4] = 3.0
    S = _sl().softmax_loss_sums(x, y.cuda())
    torch.cuda.synchronize()
    assert bool(S[1, :, 5].isnan().all()) and bool(torch.isfinite(S[0]).all()) and bool(torch.isfinite(S[1][:, [0, 1, 2, 3, 4, 6, 7]]).all())
    assert bool(torch.isnan(_sl().cross_entropy_loss(x, y.cuda())))
    cfg = SC.orch_cfg(False)
    cfg.model.loss.losses = [{"function": "CrossEntropyLoss", "target_slice": "0:1"}]
    m = ConnectomicsModule(cfg, model=torch.nn.Identity())
    with pytest.raises(FloatingPointError, match="CrossEntropyLoss is not finite"):
        m._compute_loss(x, y.cuda())
    y[1, 0, 2, 3, 4] = 2.0                                                    # a following launch on the same stream succeeds
    v = _sl().cross_entropy_loss(x, y.cuda())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(v))


# ---- nothing of the restatement runs on the device path ------------------------------------------------------------------------------------
def test_dice_ce_term_runs_no_torch_softmax_ops():
    from torch.profiler import ProfilerActivity, profile
    from pytorch_connectomics_amd.training.module import ConnectomicsModule
    cfg = SC.orch_cfg(False)
    cfg.model.loss.losses = [{"function": "DiceCELoss", "target_slice": "0:1", "kwargs": {"softmax": True, "to_onehot_y": True}}]
    m = ConnectomicsModule(cfg, model=torch.nn.Identity())
    g = torch.Generator().manual_seed(5)
    x = SC.to_layout(torch.randn(2, 3, 6, 20, 24, generator=g) * 8, "channels_last", "cuda")[0].requires_grad_(True)
    labels = torch.randint(0, 3, (2, 1, 6, 20, 24), generator=g).float().cuda()
    mask = (torch.rand(2, 1, 6, 20, 24, generator=g) > 0.3).float().cuda()

    def step():
        x.grad = None
        m._compute_loss(x, labels, mask)[0].backward()

    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    names = {e.key for e in prof.key_averages()}
    bad = sorted(n for n in names if n.startswith(BAD_OPS))
    assert not bad, bad
    assert x.grad.stride() == x.stride()                                      # dx keeps the logits' channels-last strides


# ---- refusal -------------------------------------------------------------------------------------------------------------------------------
def test_33_classes_are_refused_by_name_on_the_device_and_run_on_the_cpu():
    x = torch.zeros(1, 33, 2, 3, 4)
    y = torch.zeros(1, 1, 2, 3, 4)
    with pytest.raises(NotImplementedError, match=r"2 <= C <= 32 classes, got C = 33"):
        _sl().cross_entropy_loss(x.cuda(), y.cuda())
    with pytest.raises(NotImplementedError, match=r"got C = 33"):
        _ops().softmax_loss_forward(x.cuda(), y[:, 0].cuda())
    from pytorch_connectomics_amd import _native as nat
    import ctypes as C
    s3 = (C.c_int64 * 3)(1, 1, 1)
    p = lambda t: C.c_void_p(t.data_ptr())                                    # noqa: E731
    xd, yd, out = x.cuda(), y.cuda(), torch.zeros(33 * 8, device="cuda")
    st = nat.lib().pytc_softmax_loss_forward(p(xd), p(yd), None, p(out), p(out), 1, 33, 24, s3, s3, None, 1, -100, -20.0, None)
    assert st == nat.ERR_UNSUPPORTED
    assert float(_sl().cross_entropy_loss(x, y)) == pytest.approx(float(np.log(33.0)), rel=1e-6)
    assert bool(torch.isfinite(_sl().cross_entropy_loss(x.cuda(), y.cuda(), use_hip=False)))


# ---- the tutorial --------------------------------------------------------------------------------------------------------------------------
def test_cli_trains_the_multiclass_tutorial(tmp_path):
    """tutorials/minimal_multiclass.yaml with its output directory moved under tmp_path and its synthetic volumes (whose labels hold
    the classes 0 and 1 only) replaced by a seeded three-class label volume and a matching image: two finite training steps."""
    from pytorch_connectomics_amd.main import main
    rng = np.random.default_rng(7)
    label = rng.integers(0, 3, size=(40, 72, 72)).astype(np.float32)
    image = (label / 2.0 + 0.1 * rng.standard_normal(label.shape)).astype(np.float32)
    np.save(tmp_path / "image.npy", image)
    np.save(tmp_path / "label.npy", label)
    text = (Path(__file__).resolve().parents[1] / "tutorials" / "minimal_multiclass.yaml").read_text()
    text = re.sub(r"(?m)^save_path: .*$", f"save_path: {tmp_path / 'out'}", text, count=1)
    assert "random://minimal/train_image" in text and "random://minimal/train_label" in text
    text = text.replace("random://minimal/train_image", str(tmp_path / "image.npy")).replace("random://minimal/train_label",
                                                                                             str(tmp_path / "label.npy"))
    cfg = tmp_path / "minimal_multiclass.yaml"
    cfg.write_text(text)
    out = main(["--config", str(cfg), "--mode", "train"])
    assert out["steps"] == 2 and np.isfinite(out["first_loss"]) and np.isfinite(out["last_loss"])
    blob = torch.load(tmp_path / "out" / "checkpoints" / "last.ckpt", weights_only=True)
    assert blob["global_step"] == 2

"""GPU checks of the regularisation losses on the HIP kernels (csrc/regularization_kernels.hip).

Tolerance.  For every case the kernels' value and gradients, the fp32 torch restatement (CPU) and the fp64 restatement (CPU) are
computed on the same inputs; the kernels' error against fp64 -- the value relatively, every gradient tensor as relative L2 and as
max |err| / max |g| -- may be at most 4 x the fp32 restatement's own error against fp64, plus a floor of 1e-6 (the restatement can
land exactly on the fp64 result).  The factor covers another summation order and expf / tanhf against torch's.  The three figures
are printed per case.

Exclusions (tests/regularization_cases.py:exclusions; decided in fp64 on the inputs alone, capped at 0.1 % of a case's voxels by the
CPU suite and again here): gradients at the corner of BinaryRegularization's clamp, and around foreground / contour edge voxels just
under the upper clamp or pooled windows whose top two edges lie within 1e-5, are left out of the ELEMENTWISE check only; the value
and the relative-L2 checks always take everything.

The code-map check runs on a foreground that is constant per plane.  With sigmoid(fg) = 0 every edge magnitude is sqrt(eps), all nine
window positions tie and the code is the first in-bounds position in (y, x) scan order: 0 in the interior, 1 in the first column, 3 in
the first row, 4 at the corner (0, 0).  With sigmoid(fg) = c > 0 the zero padding of the gradient makes the border columns and rows
edges of magnitude sqrt(c^2 + eps), the corners sqrt(2 c^2 + eps): the code is the first maximum of that three-level map, which
torch's own max-pool (return_indices) gives on an exactly representable stand-in.
"""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import regularization_cases as RC  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).parent / "golden"
FACTOR, FLOOR = 4.0, 1e-6
GUARD = 64
BAD_OPS = ("aten::sigmoid", "aten::tanh", "aten::conv3d", "aten::max_pool", "aten::log_sigmoid")


def _loss(name, **kwargs):
    from pytorch_connectomics_amd.training import regularization_autograd as ra
    return getattr(ra, name)(**kwargs)


def _run(loss_name, kwargs, inputs, mask, mode):
    """-> (value as a python float, [gradient per input, fp64 on the CPU]); mode 'hip' (CUDA tensors, the kernels), 'f32' or 'f64'
    (the torch restatement on the CPU)."""
    if mode == "hip":
        conv = lambda t: t.cuda()             # noqa: E731
        loss = _loss(loss_name, **kwargs)
    else:
        dt = torch.float64 if mode == "f64" else torch.float32
        conv = lambda t: t.to(dt)             # noqa: E731
        loss = _loss(loss_name, use_hip=False, **kwargs)
    xs = [conv(t).clone().requires_grad_(True) for t in inputs]
    v = loss(*xs) if mask is None else loss(*xs, mask=conv(mask))
    grads = torch.autograd.grad(v, xs)
    if mode == "hip":
        assert v.is_cuda and v.dtype == torch.float32 and all(g.is_cuda and g.dtype == torch.float32 for g in grads)
    return float(v.detach().double().cpu()), [g.detach().double().cpu() for g in grads]


def _rel(a, r):
    return abs(a - r) / max(abs(r), 1e-300)


def _rel_l2(a, r):
    return float((a - r).norm() / r.norm().clamp_min(1e-300))


def _max_abs(a, r, keep):
    scale = float(r.abs().max().clamp_min(1e-300))
    return float(((a - r).abs() * keep).max()) / scale if a.numel() else 0.0


def _check_against_fp64(what, hip, f32, f64, excluded):
    """the tolerance of the module docstring; prints (kernel error, restatement error, bound) per figure"""
    ek, er = _rel(hip[0], f64[0]), _rel(f32[0], f64[0])
    print(f"{what}: value {hip[0]:.9g} (fp64 {f64[0]:.12g}) rel err {ek:.3g}, restatement {er:.3g}, bound {FACTOR * er + FLOOR:.3g}")
    ok = ek <= FACTOR * er + FLOOR
    for k, (gk, gr, g64) in enumerate(zip(hip[1], f32[1], f64[1])):
        assert gk.shape == g64.shape
        if float(g64.abs().max()) == 0.0:
            print(f"{what}: grad{k} is zero in fp64; kernel max |g| {float(gk.abs().max()):.3g}")
            ok = ok and float(gk.abs().max()) == 0.0
            continue
        keep = (~excluded[k]).double()
        lk, lr = _rel_l2(gk, g64), _rel_l2(gr, g64)
        mk, mr = _max_abs(gk, g64, keep), _max_abs(gr, g64, keep)
        print(f"{what}: grad{k} rel L2 {lk:.3g}, restatement {lr:.3g}, bound {FACTOR * lr + FLOOR:.3g}; max |err| / max |g| {mk:.3g}, "
              f"restatement {mr:.3g}, bound {FACTOR * mr + FLOOR:.3g}; {int(excluded[k].sum())} of {gk.numel()} elements left out")
        ok = ok and lk <= FACTOR * lr + FLOOR and mk <= FACTOR * mr + FLOOR
    assert ok, what


@pytest.mark.parametrize("case", RC.gpu_cases(), ids=lambda c: c[0])
def test_kernels_are_within_four_times_the_fp32_restatement_error(case):
    cid, loss_name, kwargs, shape, _, _ = case
    inputs, mask = RC.gpu_case_tensors(case)
    flagged, excluded = RC.exclusions(loss_name, kwargs, inputs)
    assert float(flagged.float().mean()) <= RC.EXCLUSION_CAP, (cid, int(flagged.sum()))
    hip = _run(loss_name, kwargs, inputs, mask, "hip")
    _check_against_fp64(cid, hip, _run(loss_name, kwargs, inputs, mask, "f32"), _run(loss_name, kwargs, inputs, mask, "f64"), excluded)
    if loss_name == "NonOverlapRegularization":
        assert torch.equal(hip[1][0][:, 2:], torch.zeros_like(hip[1][0][:, 2:])), "gradient outside channels 0 and 1"
        assert float(hip[1][0][:, :2].abs().max()) > 0.0
    again = _run(loss_name, kwargs, inputs, mask, "hip")                      # bit-reproducible
    assert again[0] == hip[0] and all(torch.equal(a, b) for a, b in zip(again[1], hip[1]))


# ---- the C ABI with NaN-guarded buffers ---------------------------------------------------------------------------------------------
def _guarded_out(shape, dtype):
    n = int(np.prod(shape))
    fill = float("nan") if dtype.is_floating_point else 255
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf[GUARD:GUARD + n].view(shape), buf


def _guarded_in(t, shift):
    """the operand on the device with NaN on both sides; shift 1 moves it off the 16-byte grid (the scalar path of the streaming kernels)"""
    n = t.numel()
    buf = torch.full((n + 2 * GUARD + shift,), float("nan"), dtype=torch.float32, device="cuda")
    v = buf[GUARD + shift:GUARD + shift + n].view(t.shape)
    v.copy_(t)
    return v


def _guards_ok(buf, what):
    if buf.dtype.is_floating_point:
        assert bool(buf[:GUARD].isnan().all()), f"{what}: wrote BEFORE the tensor"
        assert bool(buf[-GUARD:].isnan().all()), f"{what}: wrote PAST the tensor"
        assert not bool(buf[GUARD:-GUARD].isnan().any()), f"{what}: {int(buf[GUARD:-GUARD].isnan().sum())} elements have no writer (or are NaN)"
    else:
        assert bool((buf[:GUARD] == 255).all()), f"{what}: wrote BEFORE the tensor"
        assert bool((buf[-GUARD:] == 255).all()), f"{what}: wrote PAST the tensor"
        assert bool((buf[GUARD:-GUARD] <= 8).all()), f"{what}: {int((buf[GUARD:-GUARD] > 8).sum())} codes have no writer"


def _abi(loss_name, kwargs, inputs, mask, shift):
    """forward and backward through the C ABI as hip_ops calls them -> (sum / numel, [gradients], code or None); every output lies in
    a guarded buffer and every operand between NaNs"""
    from pytorch_connectomics_amd import _native as nat
    from pytorch_connectomics_amd import hip_ops as ops
    lib = nat.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None        # noqa: E731
    xs = [_guarded_in(t, shift) for t in inputs]
    m = _guarded_in(mask, shift) if mask is not None else None
    shape = tuple(inputs[0].shape)
    N, Cc = shape[:2]
    V = int(np.prod(shape[2:]))
    bufs = {}
    total, bufs["sum"] = _guarded_out((1,), torch.float32)
    code = None
    if loss_name == "ForegroundContourConsistency":
        D, H, W = shape[2:]
        eps = float(kwargs.get("eps", 1e-7))
        numel = N * V
        coef = torch.full((1,), 1.0, device="cuda") / float(numel)
        part, bufs["partial"] = _guarded_out((N * lib.pytc_fgcontour_tiles(D, H, W),), torch.float32)
        code, bufs["code"] = _guarded_out(shape, torch.uint8)
        grads = []
        for name in ("dfg", "dcontour"):
            g, bufs[name] = _guarded_out(shape, torch.float32)
            grads.append(g)
        nat.check(lib.pytc_fgcontour_forward(p(xs[0]), p(xs[1]), p(m), p(code), p(part), p(total), N, D, H, W, eps, st), "fgcontour_forward")
        nat.check(lib.pytc_fgcontour_backward(p(xs[0]), p(xs[1]), p(m), p(code), p(coef), p(grads[0]), p(grads[1]), N, D, H, W, eps, st),
                  "fgcontour_backward")
    else:
        kind = {"BinaryRegularization": "binary", "ForegroundDistanceConsistency": "fg_dist", "ContourDistanceConsistency": "ct_dist",
                "NonOverlapRegularization": "nonoverlap"}[loss_name]
        k = ops.REG_KINDS[kind]
        if kind == "binary":
            param, flag = float(kwargs.get("min_threshold", 1e-2)), int(kwargs.get("apply_sigmoid", True))
        else:
            param, flag = 0.0, int(kwargs.get("cleft_masked", True))
        nvol = N if kind == "nonoverlap" else N * Cc
        numel = nvol * V
        coef = torch.full((1,), 1.0, device="cuda") / float(numel)
        wC = int(mask.shape[1]) if mask is not None else Cc
        part, bufs["partial"] = _guarded_out((nvol * lib.pytc_reg_tiles(V),), torch.float32)
        grads = []
        for name in ("da", "db")[:len(xs)]:
            g, bufs[name] = _guarded_out(shape, torch.float32)
            grads.append(g)
        a, b = xs[0], (xs[1] if len(xs) == 2 else None)
        nat.check(lib.pytc_reg_pointwise_forward(k, p(a), p(b), p(m), p(part), p(total), N, Cc, wC, V, param, flag, st), "reg_forward")
        nat.check(lib.pytc_reg_pointwise_backward(k, p(a), p(b), p(m), p(coef), p(grads[0]), p(grads[1]) if b is not None else None, N, Cc,
                                                  wC, V, param, flag, st), "reg_backward")
    torch.cuda.synchronize()
    for name, buf in bufs.items():
        _guards_ok(buf, f"{loss_name} {shape} {name}")
    return (total / float(numel)).reshape(()), grads, code


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "off_by_one_float"])
@pytest.mark.parametrize("case", RC.gpu_cases(), ids=lambda c: c[0])
def test_guarded_abi_calls_equal_the_autograd_path(case, shift):
    """every output element has a writer, nothing is written (or, NaN-visibly, read) outside the tensors, and the result is bit for bit
    that of the loss class -- on 16-byte aligned operands and on operands one float off the grid"""
    cid, loss_name, kwargs, _, _, _ = case
    inputs, mask = RC.gpu_case_tensors(case)
    value, grads, _ = _abi(loss_name, kwargs, inputs, mask, shift)
    xs = [t.cuda().requires_grad_(True) for t in inputs]
    loss = _loss(loss_name, **kwargs)
    v = loss(*xs) if mask is None else loss(*xs, mask=mask.cuda())
    want = torch.autograd.grad(v, xs)
    if shift == 0:
        assert torch.equal(value, v.detach()), (cid, float(value), float(v))
    else:                                             # the scalar path deals the voxels to the threads differently: another summation order
        assert float(value) == pytest.approx(float(v), rel=1e-6), (cid, float(value), float(v))
    for k, (g, w) in enumerate(zip(grads, want)):
        assert torch.equal(g, w), (cid, k, float((g - w).abs().max()))


# ---- the code map, exactly -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RC.GPU_SHAPES_1C, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("level", ["zero", "positive"])
def test_code_map_on_a_plane_constant_foreground_is_the_first_maximum(shape, level):
    from pytorch_connectomics_amd import hip_ops as ops
    g = torch.Generator().manual_seed(sum(shape))
    N, _, D, H, W = shape
    if level == "zero":
        fg = torch.full(shape, -200.0)                                      # sigmoid = 0 exactly
    else:
        fg = (torch.rand(N, 1, D, 1, 1, generator=g) * 4.0 - 2.0).expand(shape).contiguous()
    contour = torch.randn(shape, generator=g) * 1.5
    _, code = ops.fgcontour_forward(fg.cuda(), contour.cuda(), None)
    ys, xs = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    if level == "zero":
        want = ((ys == 0).long() * 3 + (xs == 0).long()).expand(N, 1, D, H, W)
    else:
        # border columns carry |ex| = c (W > 1), border rows |ey| = c (H > 1): levels 0 / 1 / 2, pooled by torch with its own tie rule
        lvl = (((xs == 0) | (xs == W - 1)) & (W > 1)).float() + (((ys == 0) | (ys == H - 1)) & (H > 1)).float()
        pad = torch.nn.functional.pad(lvl.view(1, 1, H, W), (1, 1, 1, 1), value=-1.0)
        _, idx = torch.nn.functional.max_pool2d(pad, 3, 1, return_indices=True)
        iy, ix = idx.view(H, W) // (W + 2) - 1, idx.view(H, W) % (W + 2) - 1          # the winner in plane coordinates
        want = ((iy - ys + 1) * 3 + (ix - xs + 1)).expand(N, 1, D, H, W)
    assert code.dtype == torch.uint8 and torch.equal(code.cpu().long(), want), (shape, level)


# ---- nothing of the restatement runs on the device path --------------------------------------------------------------------------------
def _profiled_ops(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()                                                                     # warm-up (library load)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.key for e in prof.key_averages()}


@pytest.mark.parametrize("name", RC.LOSSES)
def test_forward_and_backward_run_no_torch_restatement_ops(name):
    shape = (2, 3, 6, 20, 24) if name == "NonOverlapRegularization" else (2, 1, 6, 20, 24)
    xs = [torch.randn(shape, device="cuda", requires_grad=True) for _ in range(RC.N_INPUTS[name])]
    mask = torch.rand(shape, device="cuda") if RC.TAKES_MASK[name] else None
    loss = _loss(name)

    def step():
        (loss(*xs) if mask is None else loss(*xs, mask=mask)).backward()

    names = _profiled_ops(step)
    bad = sorted(n for n in names if n.startswith(BAD_OPS))
    assert not bad, bad


def _cfg(terms, heads=None, ds=False):
    from types import SimpleNamespace as NS
    return NS(model=NS(loss=NS(deep_supervision=ds, deep_supervision_weights=[1.0], deep_supervision_clamp_min=-20.0,
                               deep_supervision_clamp_max=20.0, losses=terms, loss_balancing=None, fused=True),
                       primary_head=None, heads=heads, out_channels=2), data=NS(label_transform=None), optimization=NS())


def test_regulariser_keeps_the_supervised_terms_on_the_fused_kernel():
    from pytorch_connectomics_amd.training.module import ConnectomicsModule, dice_loss_sigmoid, weighted_bce_with_logits
    terms = [{"function": "WeightedBCEWithLogitsLoss", "weight": 1.0}, {"function": "DiceLoss", "weight": 0.5, "kwargs": {"sigmoid": True}},
             {"function": "BinaryRegularization", "weight": 0.01, "pred_slice": "0:2"}]
    m = ConnectomicsModule(_cfg(terms), model=torch.nn.Identity())
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(2, 2, 6, 20, 24, generator=g) * 3
    y = (torch.rand(2, 2, 6, 20, 24, generator=g) > 0.5).float()
    x = x0.cuda().requires_grad_(True)
    yc = y.cuda()

    def step():
        x.grad = None
        m._compute_loss(x, yc)[0].backward()

    names = _profiled_ops(step)
    bad = sorted(n for n in names if n.startswith(("aten::binary_cross_entropy_with_logits",) + BAD_OPS))
    assert not bad, bad
    total, parts = m._compute_loss(x, yc)
    xd = x0.double()
    want = weighted_bce_with_logits(x0, y).double() + 0.5 * dice_loss_sigmoid(x0, y).double() + \
        0.01 * _loss("BinaryRegularization", use_hip=False)(xd)
    assert float(total) == pytest.approx(float(want), rel=1e-5)
    assert sorted(parts) == ["loss_0_WeightedBCEWithLogitsLoss", "loss_1_DiceLoss", "loss_2_BinaryRegularization", "train_loss_total"]


# ---- the reference fixtures on the device ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_fixture_cases_on_the_device(name):
    """the reference's own fp32 value and gradients stand for the fp32 restatement (the CPU suite shows they are bit-identical)"""
    gold = np.load(GOLD / "regularization.npz")
    loss_name, kwargs = RC.CASES[name][:2]
    inputs = [torch.from_numpy(gold[f"{name}__in{k}"]) for k in range(RC.N_INPUTS[loss_name])]
    mask = torch.from_numpy(gold[f"{name}__mask"]) if f"{name}__mask" in gold.files else None
    ref = (float(gold[f"{name}__loss"]), [torch.from_numpy(gold[f"{name}__grad{k}"]).double() for k in range(len(inputs))])
    _, excluded = RC.exclusions(loss_name, kwargs, inputs)
    _check_against_fp64(name, _run(loss_name, kwargs, inputs, mask, "hip"), ref, _run(loss_name, kwargs, inputs, mask, "f64"), excluded)


@pytest.mark.parametrize("which", sorted(RC.ORCH_TERMS))
def test_orchestrator_fixtures_on_the_device(which):
    """ConnectomicsModule on CUDA tensors against the reference orchestrator's total and gradients.  The fp64 yardstick is the module on
    fp64 CPU tensors: the regularisers run in fp64 there, the supervised terms of the module compute in fp32 whatever they are given, so
    for their share the bound is no wider than the floor."""
    from pytorch_connectomics_amd.training.module import ConnectomicsModule
    gold = np.load(GOLD / "regularization.npz")
    pre = f"orch_{which}__"
    names = [k[len(pre) + 3:] for k in gold.files if k.startswith(pre + "in_")]
    m = ConnectomicsModule(RC.orch_cfg(which), model=torch.nn.Identity())

    def run(conv):
        outs = {k: conv(torch.from_numpy(gold[f"{pre}in_{k}"])).requires_grad_(True) for k in names}
        model_out = outs["output"] if which == "plain" else dict(outs)
        total, _ = m._compute_loss(model_out, conv(torch.from_numpy(gold[pre + "labels"])), conv(torch.from_numpy(gold[pre + "mask"])))
        grads = torch.autograd.grad(total, [outs[k] for k in names])
        return float(total.detach().double().cpu()), [g.detach().double().cpu() for g in grads]

    ref = (float(gold[pre + "total"]), [torch.from_numpy(gold[f"{pre}grad_{k}"]).double() for k in names])
    hip, f64 = run(lambda t: t.cuda()), run(lambda t: t.double())
    _check_against_fp64(f"orchestrator {which}", hip, ref, f64, [torch.zeros_like(g, dtype=torch.bool) for g in ref[1]])


def test_cli_trains_the_regularized_tutorial(tmp_path):
    """tutorials/minimal_regularized.yaml as committed (only its output directory moved under tmp_path): two finite training steps."""
    from pytorch_connectomics_amd.main import main
    text = (Path(__file__).resolve().parents[1] / "tutorials" / "minimal_regularized.yaml").read_text()
    cfg = tmp_path / "minimal_regularized.yaml"
    cfg.write_text(re.sub(r"(?m)^save_path: .*$", f"save_path: {tmp_path / 'out'}", text, count=1))
    out = main(["--config", str(cfg), "--mode", "train"])
    assert out["steps"] == 2 and np.isfinite(out["first_loss"])
    blob = torch.load(tmp_path / "out" / "checkpoints" / "last.ckpt", weights_only=True)
    assert blob["global_step"] == 2

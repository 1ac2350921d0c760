"""The sliding-window and volume-reader kernels (csrc/window_kernels.hip, csrc/volume_kernels.hip) against the CPU model of
tests/window_kernel_model.py, called directly through their hip_ops wrappers.

These kernels are written with explicit roundings, one writer per element and windows in stream order, so plain fp32 array arithmetic
reproduces them bit for bit: every comparison here is on the BITS of every element (no voxel is left out), except the activations
(device expf / tanhf), which are held to FACTOR x the error of the same model evaluated in fp32 on the CPU, both measured against the
model in fp64.  Outputs and accumulators live between guard words; the shapes (tests/window_exact_shapes.py, checked on the CPU by
tests/test_host_window_kernel_model.py) are the smallest at which the kernels can still go wrong: more than one workgroup with a
ragged last one, windows overhanging every face, and the sizes at which the grid-stride loops take a second trip."""
import itertools

import numpy as np
import pytest
import torch

import window_exact_shapes as SH
from oracle import window_oracle as WO
from pytorch_connectomics_amd import _native as nat
from window_kernel_model import KernelModel as M
from window_kernel_model import LEGAL_VIEWS, legal_views

pytestmark = pytest.mark.gpu

FACTOR, FLOOR = 4.0, 1e-6          # tests/test_gpu_softmax_losses.py
GUARD = 64                         # guard words on either side (256 bytes: float4 alignment is kept)
ROIS = [w for w, _ in SH.WINDOWS]
_INT = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from pytorch_connectomics_amd import hip_ops
    return hip_ops


# ---- helpers -------------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(*shape, seed):
    return torch.randn(*shape, generator=_gen(seed))


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(_INT[t.element_size()])


def _same(got, want, what):
    """every element, bit for bit"""
    got = got.detach().cpu()
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), f"{what}: {got.dtype} {tuple(got.shape)} vs {want.dtype} {tuple(want.shape)}"
    g, w = _bits(got), _bits(want)
    if not torch.equal(g, w):
        bad = torch.nonzero(g != w)
        k = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.numel()} elements differ; first at {k}: device {got[k].item()!r}, model {want[k].item()!r}")


class Guarded:
    """a device tensor holding `src` between NaN guard words"""

    def __init__(self, src):
        n = src.numel()
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=src.dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + n].view(src.shape)
        self.t.copy_(src)

    @classmethod
    def empty(cls, shape, dtype=torch.float32):
        """all NaN: an element that is still NaN afterwards had no writer"""
        return cls(torch.full(tuple(shape), float("nan"), dtype=dtype))

    def clone(self):
        """a second allocation with the same contents, copied on the device"""
        other = object.__new__(Guarded)
        other.buf = self.buf.clone()
        other.t = other.buf[GUARD:GUARD + self.t.numel()].view(self.t.shape)
        return other

    def intact(self):
        return bool(self.buf[:GUARD].isnan().all()) and bool(self.buf[-GUARD:].isnan().all())


def _bump(roi):
    from pytorch_connectomics_amd.inference.window import _axis_kernels
    ks, comb = _axis_kernels(roi, "bump", torch.float32)
    assert comb == nat.BLEND_PRODUCT
    return [k.contiguous() for k in ks]


def _random_weights(roi, seed):
    g = _gen(seed)
    return [torch.rand(n, generator=g) * 1.5 + 0.05 for n in roi]


def _cuda(ts):
    return [t.cuda() for t in ts]


# ---- gather_windows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("roi", ROIS, ids=str)
def test_gather_every_view_code_in_both_dtypes(ops, roi):
    """all 32 view codes meet a window they are legal for; in-volume windows, C = 3; every output element has a writer"""
    ext = SH.volume_of(roi)
    vol = _randn(3, *ext, seed=11)
    dvol = vol.cuda()
    starts = [(0, 0, 0), tuple(e - r for e, r in zip(ext, roi)), (1, 2, 3), (3, 1, 2)]
    for view in legal_views(roi):
        for dt in (torch.float32, torch.bfloat16):
            out = Guarded.empty((len(starts), *roi, 3), dt)
            got = ops.gather_windows(dvol, starts, roi, view=view, out_dtype=dt, out=out.t)
            assert got.data_ptr() == out.t.data_ptr()
            _same(got, M.gather_windows(vol, starts, roi, view=view, out_dtype=dt), f"gather view {view} {dt}")
            assert out.intact(), f"gather view {view} {dt}: a guard word was written"
            _same(ops.gather_windows(dvol, starts, roi, view=view, out_dtype=dt), got.cpu(), f"gather view {view} {dt} (own output)")


def _pad_windows(roi, ext):
    wins = list(itertools.product(*WO.lazy_axis_offsets(ext, roi, 0.5)))
    wins += [(ext[0] - 1, 3, 4),                      # the in-volume crop is one voxel thick: reflect degrades to edge
             (-5, 2, ext[2] - 3),                     # pads longer than the crop (2 and 3 voxels of it): the periodic bounce
             (ext[0], 1, 2), (2, -roi[1] - 2, 1), (3, 3, ext[2] + 5)]     # wholly outside along z, along y, along x
    return wins


@pytest.mark.parametrize("pad_mode", ["constant", "reflect", "replicate", "circular"])
def test_gather_pad_modes_over_the_overhanging_grid(ops, pad_mode):
    """the lazy grid of overhanging starts plus the degenerate windows, every legal view code, a non-zero cval; 135 windows go in
    chunks of 64 + 64 + 7, and B = 1 / 64 / 65 once more on their own"""
    roi = (7, 7, 7)
    ext = SH.volume_of(roi)
    vol = _randn(3, *ext, seed=12)
    dvol = vol.cuda()
    wins = _pad_windows(roi, ext)
    assert len(wins) > 128
    plain = M.gather_plain(vol, wins, roi, pad_mode=pad_mode, cval=-0.75)
    out = Guarded.empty((len(wins), *roi, 3))
    for view in legal_views(roi):
        out.t.fill_(float("nan"))
        ops.gather_windows(dvol, wins, roi, view=view, pad_mode=pad_mode, cval=-0.75, out=out.t)
        _same(out.t, M.to_view(plain, view).contiguous(), f"gather {pad_mode} view {view}")
    assert out.intact()
    tail = wins[-70:]                                   # the degenerate windows are among them
    for B, view in ((1, 5), (64, 34), (65, 19)):
        o = Guarded.empty((B, *roi, 3), torch.bfloat16)
        ops.gather_windows(dvol, tail[-B:], roi, view=view, pad_mode=pad_mode, cval=-0.75, out_dtype=torch.bfloat16, out=o.t)
        _same(o.t, M.gather_windows(vol, tail[-B:], roi, view=view, pad_mode=pad_mode, cval=-0.75, out_dtype=torch.bfloat16),
              f"gather {pad_mode} B={B}")
        assert o.intact()


# ---- blend_accumulate ----------------------------------------------------------------------------------------------------------------------
def _blend_case(ops, roi, C, pred, dpred, starts, ws, dws, v0, w0, kw, *, with_weight=True, what="", templates=None):
    value, weight = (templates[0].clone(), templates[1].clone()) if templates else (Guarded(v0), Guarded(w0))
    ops.blend_accumulate(dpred, starts, value.t, weight.t if with_weight else None, *dws, **kw)
    mv, mw = v0.clone(), w0.clone()
    M.blend_accumulate(pred, starts, mv, mw if with_weight else None, *ws, **kw)
    _same(value.t, mv, f"blend value {what}")
    _same(weight.t, mw, f"blend weight {what}")            # not given: untouched
    assert value.intact() and weight.intact(), f"blend {what}: a guard word was written"
    return mv, mw


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("roi", ROIS, ids=str)
def test_blend_accumulate_every_option(ops, roi, dt):
    """{bump, random} axis weights x {PRODUCT, MIN} x floors x border x {fp32, bf16} x weight given or not x every legal view; six windows
    in list order, four of them sharing voxels, overhang on all six faces, pre-filled accumulators; uncovered voxels keep their bits"""
    C = 3
    ext, starts = SH.volume_of(roi), SH.blend_starts(roi)
    v0, w0 = _randn(C, *ext, seed=21), _randn(*ext, seed=22).abs() + 0.1
    cover = torch.zeros(ext, dtype=torch.bool)
    for s in starts:
        cover[tuple(slice(max(0, s[a]), max(0, s[a] + roi[a])) for a in range(3))] = True
    assert not bool(cover.all())
    preds = {torch.float32: _randn(len(starts), *roi, C, seed=23)}
    preds[torch.bfloat16] = preds[torch.float32].to(torch.bfloat16)
    dpreds = {k: v.cuda() for k, v in preds.items()}
    weights = {"bump": _bump(roi), "random": _random_weights(roi, 24)}
    dweights = {k: _cuda(v) for k, v in weights.items()}
    views = legal_views(roi)
    templates = Guarded(v0), Guarded(w0)
    n = 0
    for wname, combine, floor_w, border, with_weight in itertools.product(
            weights, (nat.BLEND_PRODUCT, nat.BLEND_MIN), (0.0, 1e-5, 0.5), (None, (1, 2, 0)), (True, False)):
        for view in views:
            kw = dict(view=view, combine=combine, floor_w=floor_w, border=border)
            what = f"{wname} combine {combine} floor {floor_w} border {border} {dt} weight {with_weight} view {view}"
            mv, mw = _blend_case(ops, roi, C, preds[dt], dpreds[dt], starts, weights[wname], dweights[wname], v0, w0, kw,
                                 with_weight=with_weight, what=what, templates=templates)
            assert torch.equal(_bits(mv[:, ~cover]), _bits(v0[:, ~cover])) and torch.equal(_bits(mw[~cover]), _bits(w0[~cover]))
            n += 1
    assert n == 48 * len(views)


@pytest.mark.parametrize("C", [1, 7])
def test_blend_accumulate_other_channel_counts_and_the_tiny_floor(ops, C):
    roi = (7, 7, 7)
    ext, starts = SH.volume_of(roi), SH.blend_starts(roi)
    v0, w0 = _randn(C, *ext, seed=31), _randn(*ext, seed=32).abs() + 0.1
    pred = _randn(len(starts), *roi, C, seed=33)
    ws = _random_weights(roi, 34)
    for view in LEGAL_VIEWS:
        for dt in (torch.float32, torch.bfloat16):
            p = pred.to(dt)
            _blend_case(ops, roi, C, p, p.cuda(), starts, ws, _cuda(ws), v0, w0, dict(view=view, combine=nat.BLEND_PRODUCT, floor_w=1e-5,
                                                                                     border=(1, 2, 0)), what=f"C={C} view {view} {dt}")
    # the product of the axis weights underflows to 0: the FLT_MIN floor is what every voxel gets.  Predictions in [1, 2) and zeroed
    # accumulators keep every product and sum a normal number (subnormal handling is not under test)
    tiny = [torch.full((n,), 1e-20) for n in roi]
    pred = torch.rand(len(starts), *roi, C, generator=_gen(35)) + 1.0
    z = torch.zeros(C, *ext), torch.zeros(ext)
    mv, mw = _blend_case(ops, roi, C, pred, pred.cuda(), starts, tiny, _cuda(tiny), *z, dict(view=0, combine=nat.BLEND_PRODUCT, floor_w=0.0),
                         what="FLT_MIN floor")
    flt_min = float(np.float32(1.17549435e-38))
    assert float(mw.max()) >= 4 * flt_min and set(np.unique((mw / flt_min).numpy()).tolist()) <= {0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0}
    assert float(mv[mv != 0].abs().min()) >= flt_min


# ---- blend_accumulate_mapped, blend_weight_shifted -----------------------------------------------------------------------------------------
def _chan_map(C, roi, seed):
    """a permutation that is not the identity; shifts of both signs, zero, and one at least as long as the window (its channel gets nothing)"""
    rng = np.random.default_rng(seed)
    src = list(np.roll(np.arange(C), 3 if C > 3 else 1))
    assert src != list(range(C))
    shifts = [(0, 0, 0), (1, -2, 0), (-1, 0, 3), (0, roi[1], 0), (-2, 1, -1), (0, 0, -roi[2] - 1), (2, 2, 2)]
    shifts += [tuple(int(v) for v in rng.integers(-3, 4, 3)) for _ in range(C - len(shifts))]
    return [int(v) for v in src], shifts[:C]


@pytest.mark.parametrize("C,roi", [(7, (7, 7, 7)), (7, (5, 7, 9)), (32, (7, 7, 7)), (32, (5, 8, 8))], ids=str)
def test_blend_accumulate_mapped(ops, C, roi):
    ext, starts = SH.volume_of(roi), SH.blend_starts(roi)
    src, shifts = _chan_map(C, roi, C)
    v0, w0 = _randn(C, *ext, seed=41), _randn(*ext, seed=42).abs() + 0.1
    pred = _randn(len(starts), *roi, C, seed=43)
    ws = {"bump": _bump(roi), "random": _random_weights(roi, 44)}
    views = legal_views(roi) if C == 7 else [0, legal_views(roi)[-1]]
    assert 0 in views and len(views) > 1
    for view, dt, (wname, combine, floor_w, border), with_weight in itertools.product(
            views, (torch.float32, torch.bfloat16),
            (("bump", nat.BLEND_PRODUCT, 1e-5, None), ("random", nat.BLEND_MIN, 0.0, (1, 2, 0)), ("random", nat.BLEND_PRODUCT, 0.5, (1, 2, 0))),
            (True, False)):
        kw = dict(view=view, combine=combine, floor_w=floor_w, border=border)
        what = f"mapped C={C} view {view} {dt} {wname} combine {combine} weight {with_weight}"
        p = pred.to(dt)
        value, weight = Guarded(v0), Guarded(w0)
        ops.blend_accumulate_mapped(p.cuda(), starts, value.t, weight.t if with_weight else None, *_cuda(ws[wname]), src, shifts, **kw)
        mv, mw = v0.clone(), w0.clone()
        M.blend_accumulate_mapped(p, starts, mv, mw if with_weight else None, *ws[wname], src, shifts, **kw)
        _same(value.t, mv, what + " value")
        _same(weight.t, mw, what + " weight")
        assert value.intact() and weight.intact()
        gone = [d for d, s in enumerate(shifts) if any(abs(s[a]) >= roi[a] for a in range(3))]
        assert gone and all(torch.equal(_bits(mv[d]), _bits(v0[d])) for d in gone)          # a channel shifted out of the window gets nothing
        if with_weight:                                                                      # the weight lands at the unshifted positions
            pw = w0.clone()
            M.blend_accumulate(p[..., :1], starts, torch.zeros(1, *ext), pw, *ws[wname], **kw)
            assert torch.equal(_bits(mw), _bits(pw))


@pytest.mark.parametrize("roi", [(5, 7, 9), (7, 7, 7)], ids=str)
def test_blend_weight_shifted(ops, roi):
    ext, starts = SH.volume_of(roi), SH.blend_starts(roi)
    w0 = _randn(*ext, seed=51).abs() + 0.1
    ws = {"bump": _bump(roi), "random": _random_weights(roi, 52)}
    three = [starts[0], starts[2], starts[3]]                      # B = 3: two overlapping windows and the one over the low faces
    for st, shift, (wname, combine, floor_w, border) in itertools.product(
            (three, starts), ((0, 0, 0), (1, -2, 3), (-2, 0, -1), (0, roi[1], 0), (roi[0] - 1, 1 - roi[1], 0)),
            (("bump", nat.BLEND_PRODUCT, 1e-5, None), ("random", nat.BLEND_MIN, 0.0, (1, 2, 0)), ("random", nat.BLEND_PRODUCT, 0.5, (1, 2, 0)))):
        kw = dict(combine=combine, floor_w=floor_w, border=border)
        weight = Guarded(w0)
        ops.blend_weight_shifted(st, roi, weight.t, *_cuda(ws[wname]), shift, **kw)
        mw = w0.clone()
        M.blend_weight_shifted(st, roi, mw, *ws[wname], shift, **kw)
        _same(weight.t, mw, f"weight_shifted B={len(st)} shift {shift} {wname} combine {combine}")
        assert weight.intact()


def test_blend_refusals_come_before_any_launch(ops):
    roi = (7, 7, 7)
    ext, starts = SH.volume_of(roi), SH.blend_starts(roi)
    ws = _cuda(_random_weights(roi, 61))

    def refused(C, call, exc=(RuntimeError, ValueError), match=None):
        v0, w0 = _randn(C, *ext, seed=62), _randn(*ext, seed=63)
        value, weight = Guarded(v0), Guarded(w0)
        with pytest.raises(exc, match=match):
            call(value.t, weight.t)
        torch.cuda.synchronize()
        _same(value.t, v0, "refused call: value")
        _same(weight.t, w0, "refused call: weight")

    p33 = _randn(len(starts), *roi, 33, seed=64).cuda()
    refused(33, lambda v, w: ops.blend_accumulate_mapped(p33, starts, v, w, *ws, list(range(33)), [(0, 0, 0)] * 33), match="must be in")
    p3 = _randn(len(starts), *roi, 3, seed=65).cuda()
    ident = ([0, 1, 2], [(0, 0, 0)] * 3)
    for fn, extra in ((ops.blend_accumulate, ()), (ops.blend_accumulate_mapped, ident)):
        refused(3, lambda v, w: fn(p3, starts, v, w, *ws, *extra, view=nat.VIEW_SWAP_YX | nat.VIEW_SWAP_ZX), match="SWAP")
        refused(3, lambda v, w: fn(p3, starts, v, w, *ws, *extra, border=(0, 0, 4)), match="border")       # 2 * 4 >= 7: over half the window
        refused(3, lambda v, w: fn(p3, starts, v, w, *ws, *extra, combine=2), match="combine")
    roi2 = (5, 8, 8)                                                # half the window exactly
    p2 = _randn(1, *roi2, 3, seed=66).cuda()
    ws2 = _cuda(_random_weights(roi2, 67))
    refused(3, lambda v, w: ops.blend_accumulate(p2, [(0, 0, 0)], v, w, *ws2, border=(0, 4, 0)), match="border")
    refused(3, lambda v, w: ops.blend_accumulate(p2, [(0, 0, 0)], v, w, *ws2, view=nat.VIEW_SWAP_ZY), match="equal length")   # 5 != 8
    refused(3, lambda v, w: ops.blend_accumulate(p2, [(0, 0, 0)], v, w, *ws2, view=nat.VIEW_SWAP_ZX | nat.VIEW_FLIP_X), match="equal length")
    for kw, match in ((dict(combine=2), "combine"), (dict(border=(0, 0, 4)), "border"), (dict(border=(-1, 0, 0)), "border")):
        refused(1, lambda v, w: ops.blend_weight_shifted(starts, roi, w, *ws, (1, 0, -1), **kw), match=match)
    refused(1, lambda v, w: ops.blend_weight_shifted([(0, 0, 0)], roi2, w, *ws2, (0, 0, 0), border=(0, 4, 0)), match="border")
    vol = _randn(3, *ext, seed=68).cuda()
    for view in (nat.VIEW_SWAP_YX | nat.VIEW_SWAP_ZY, 64):
        with pytest.raises(RuntimeError, match="SWAP"):
            ops.gather_windows(vol, starts, roi, view=view)
    with pytest.raises(RuntimeError, match="equal length"):
        ops.gather_windows(vol, [(0, 0, 0)], roi2, view=nat.VIEW_SWAP_ZY)


# ---- operand checks of the wrappers (no kernel runs) ----------------------------------------------------------------------------------------
def test_wrappers_refuse_operands_the_kernels_would_read_out_of_bounds(ops):
    roi = (5, 7, 9)
    ext = SH.volume_of(roi)
    pred = torch.zeros(1, *roi, 3, device="cuda")
    value, weight = torch.zeros(3, *ext, device="cuda"), torch.zeros(ext, device="cuda")
    ws = [torch.ones(n, device="cuda") for n in roi]
    ident = ([0, 1, 2], [(0, 0, 0)] * 3)
    st = [(0, 0, 0)]
    bad_weights = [torch.zeros(ext[0], ext[1], ext[2] - 1, device="cuda"), torch.zeros(ext, device="cuda", dtype=torch.float64),
                   torch.zeros(ext[0], ext[1], 2 * ext[2], device="cuda")[..., ::2], torch.zeros(ext), torch.zeros(ext, device="cuda").view(-1)]

    def bad_vectors(n):
        """too short, too long, not fp32, strided, on the host, not a vector, missing"""
        return [torch.ones(n - 1, device="cuda"), torch.ones(n + 1, device="cuda"), torch.ones(n, device="cuda", dtype=torch.float64),
                torch.ones(2 * n, device="cuda")[::2], torch.ones(n), torch.ones(1, n, device="cuda"), None]

    for fn, extra in ((ops.blend_accumulate, ()), (ops.blend_accumulate_mapped, ident)):
        for bw in bad_weights:
            with pytest.raises(ValueError, match="weight"):
                fn(pred, st, value, bw, *ws, *extra)
        for k, name in enumerate(("wz", "wy", "wx")):
            for bv in bad_vectors(roi[k]):
                v3 = list(ws)
                v3[k] = bv
                with pytest.raises(ValueError, match=name):
                    fn(pred, st, value, weight, *v3, *extra)
        fn(pred, st, value, None, *ws, *extra)                      # weight = None is legal
    for bw in bad_weights[1:3] + bad_weights[4:]:                   # not fp32; strided; not (Z, Y, X)
        with pytest.raises(ValueError):
            ops.blend_weight_shifted(st, roi, bw, *ws, (0, 0, 0))
    with pytest.raises(RuntimeError, match="no CPU path"):          # a host accumulator: the refusal every wrapper of the package gives
        ops.blend_weight_shifted(st, roi, bad_weights[3], *ws, (0, 0, 0))
    for k, name in enumerate(("wz", "wy", "wx")):
        for bv in bad_vectors(roi[k]):
            v3 = list(ws)
            v3[k] = bv
            with pytest.raises(ValueError, match=name):
                ops.blend_weight_shifted(st, roi, weight, *v3, (0, 0, 0))
    assert float(value.abs().sum()) == 0.0 and float(weight.abs().sum()) == 0.0
    # blend_finalize: fp32 operands with value.numel() == C * weight.numel()
    with pytest.raises(ValueError):
        ops.blend_finalize(value, weight.view(-1)[:-1])
    with pytest.raises(ValueError):
        ops.blend_finalize(value, weight.double())
    with pytest.raises(ValueError):
        ops.blend_finalize(value.double(), weight)
    with pytest.raises(ValueError):
        ops.blend_finalize(torch.zeros(3, ext[0] * ext[1] * ext[2] + 1, device="cuda"), weight)
    with pytest.raises(ValueError):
        ops.blend_finalize(value, bad_weights[2])                   # strided
    with pytest.raises(ValueError):
        ops.blend_finalize(torch.zeros(3, *ext, 2, device="cuda")[..., 0], weight)
    for args in ((value.cpu(), weight), (value, weight.cpu())):
        with pytest.raises(RuntimeError, match="no CPU path"):
            ops.blend_finalize(*args)
    # the ensemble wrappers: fp32, contiguous, equal numel for every operand given
    a = torch.zeros(100, device="cuda")
    short, dbl, strided = torch.zeros(99, device="cuda"), torch.zeros(100, device="cuda", dtype=torch.float64), torch.zeros(200, device="cuda")[::2]
    host = torch.zeros(100)                                         # a host tensor: the refusal every wrapper of the package gives
    for fn, n_ops, tail in ((ops.ensemble_update, 2, (0, 2)), (ops.ensemble_update_masked, 4, (0,)), (ops.ensemble_finalize_masked, 3, (0,))):
        for k in range(n_ops):
            args = [a] * n_ops
            args[k] = host
            with pytest.raises(RuntimeError, match="no CPU path"):
                fn(*args, *tail)
    for bad in (short, dbl, strided):                               # on the device: the wrong size, dtype, layout
        for args in ((bad, a), (a, bad)):
            with pytest.raises(ValueError):
                ops.ensemble_update(*args, 0, 2)
        for args in ((bad, a, a, a), (a, bad, a, a), (a, a, bad, a), (a, a, a, bad), (a, bad, a, None)):
            with pytest.raises(ValueError):
                ops.ensemble_update_masked(*args, 0)
        for args in ((bad, a, a), (a, bad, a), (a, a, bad)):
            with pytest.raises(ValueError):
                ops.ensemble_finalize_masked(*args, 0)
    assert float(a.abs().sum()) == 0.0
    # gather_windows: a caller-supplied out
    vol = torch.zeros(3, *ext, device="cuda")
    for bad in (torch.empty(1, *roi, 2, device="cuda"), torch.empty(2, *roi, 3, device="cuda"), torch.empty(1, *roi, 3, device="cuda", dtype=torch.float16),
                torch.empty(1, *roi, 6, device="cuda")[..., ::2], torch.empty(1, *roi, 3), torch.empty(1, roi[0], roi[2], roi[1], 3, device="cuda")):
        with pytest.raises(ValueError, match="out"):
            ops.gather_windows(vol, st, roi, out=bad)


# ---- flat elementwise kernels ------------------------------------------------------------------------------------------------------------------
def _flat(n, seed):
    return _randn(n, seed=seed)


@pytest.mark.parametrize("n", SH.FLAT_SIZES)
def test_normalize_covered_and_blend_finalize(ops, n):
    """weights that are zero, negative and positive; weights below, at and above the clamp; the last size sends every grid-stride loop
    on a second trip"""
    g = _gen(71)
    v0 = _flat(n, 72)
    w0 = torch.tensor([0.0, -1.5, 0.75, 2.0, 1e-3])[torch.randint(0, 5, (n,), generator=g)] * (torch.rand(n, generator=g) + 0.5)
    value, weight = Guarded(v0), Guarded(w0)
    ops.normalize_covered(value.t, weight.t)
    mv = v0.clone()
    M.normalize_covered(mv, w0)
    _same(value.t, mv, f"normalize_covered n={n}")
    _same(weight.t, w0, "normalize_covered weight")
    assert value.intact() and weight.intact()
    clamp = 1e-4
    c32 = float(np.float32(clamp))
    for C in (1, 3):
        v0 = _randn(C, n, seed=73)
        w0 = torch.tensor([0.0, 0.5 * c32, c32, 2 * c32, 1.0, 3.0])[torch.randint(0, 6, (n,), generator=g)]
        value, weight = Guarded(v0), Guarded(w0)
        ops.blend_finalize(value.t, weight.t, clamp=clamp)
        mv = v0.clone()
        M.blend_finalize(mv, w0, clamp=clamp)
        _same(value.t, mv, f"blend_finalize n={n} C={C}")
        assert value.intact() and weight.intact()


@pytest.mark.parametrize("n", SH.FLAT_SIZES)
def test_ensemble_kernels(ops, n):
    """five updates per mode; the masked form with covers of zeros, negatives and NaNs and with cover = None, every voxel covered by the
    first update; finalize in a guarded output"""
    xs = [_flat(n, 80 + i) for i in range(5)]
    for mode in (0, 1, 2):
        acc = Guarded(_flat(n, 79))
        macc = _flat(n, 79)
        for i, x in enumerate(xs):
            ops.ensemble_update(acc.t, x.cuda(), mode, i + 1)
            M.ensemble_update(macc, x, mode, i + 1)
        _same(acc.t, macc, f"ensemble_update mode {mode} n={n}")
        assert acc.intact()
        g = _gen(90 + mode)
        covers = [torch.ones(n), None] + [torch.tensor([1.0, 0.0, -1.0, float("nan"), 2.5])[torch.randint(0, 5, (n,), generator=g)] for _ in range(3)]
        s0 = torch.zeros(n) if mode == 0 else torch.full((n,), float("inf") if mode == 1 else float("-inf"))
        stat, count, out = Guarded(s0), Guarded(torch.zeros(n)), Guarded.empty((n,))
        ms, mc, mo = s0.clone(), torch.zeros(n), torch.empty(n)
        for x, cv in zip(xs, covers):
            ops.ensemble_update_masked(stat.t, count.t, x.cuda(), None if cv is None else cv.cuda(), mode)
            M.ensemble_update_masked(ms, mc, x, cv, mode)
        _same(stat.t, ms, f"ensemble_update_masked stat mode {mode} n={n}")
        _same(count.t, mc, f"ensemble_update_masked count mode {mode} n={n}")
        assert float(mc.min()) >= 2.0 and (n < 255 or float(mc.max()) > float(mc.min()))
        ops.ensemble_finalize_masked(stat.t, count.t, out.t, mode)
        M.ensemble_finalize_masked(ms, mc, mo, mode)
        _same(out.t, mo, f"ensemble_finalize_masked mode {mode} n={n}")
        assert stat.intact() and count.intact() and out.intact()


# ---- scale_cast ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target,scale", [("uint8", 255.0), ("int8", 100.0), ("uint16", 65535.0), ("int16", 3e4), ("int32", 2e9), ("float16", 5e4),
                                          ("float32", 2.5), ("uint8", -1.0)])
def test_scale_cast_every_target_tail_and_stride(ops, target, scale):
    """four elements per thread: n below four, one / two / three elements of scalar tail, and a size above the 8192-block cap; inputs in
    [-1.3, 1.6) clip at both ends of every integer target"""
    for n in SH.CAST_SIZES:
        x = torch.rand(n, generator=_gen(n % 1000)) * 2.9 - 1.3
        if n >= 5:
            x[:5] = torch.tensor([-1.3, 1.6, 0.0, 0.999999, -0.999999])
        got = ops.scale_cast(x.cuda(), scale=scale, target=target)
        _same(got, M.scale_cast(x, scale=scale, target=target), f"scale_cast {target} n={n}")


# ---- window_normalize ----------------------------------------------------------------------------------------------------------------------
def _integer_windows(n):
    rng = np.random.default_rng(101)
    x = np.stack([rng.integers(0, 256, n), rng.integers(40, 90, n), np.full(n, 7)]).astype(np.float32)
    return torch.from_numpy(x)


NORM_CASES = {"zscore": dict(mode=nat.NORM_ZSCORE), "minmax": dict(mode=nat.NORM_MINMAX), "divide": dict(mode=nat.NORM_DIVIDE, divide=255.0),
              "binarise+zscore": dict(mode=nat.NORM_ZSCORE, binarize=True, threshold=60.0), "clip+zscore": dict(mode=nat.NORM_ZSCORE, clip=True)}


@pytest.mark.parametrize("case", list(NORM_CASES))
def test_window_normalize_integer_windows_exactly(ops, case):
    """three windows of 2 * 8192 + 37 values (three statistics slots, the last ragged), integer valued so that the fp64 sums are exact
    in any order, one window constant: the device equals the model bit for bit, twice"""
    kw = dict(NORM_CASES[case])
    x = _integer_windows(SH.NORM_N)
    clip = torch.tensor([[10.0, 200.0], [50.0, 80.0], [0.0, 5.0]]) if kw.pop("clip", False) else None
    want = M.window_normalize(x.clone(), clip=clip, **kw)
    runs = []
    for _ in range(2):
        g = Guarded(x)
        ops.window_normalize(g.t, clip=None if clip is None else clip.cuda(), **kw)
        _same(g.t, want, f"window_normalize {case}")
        assert g.intact()
        runs.append(g.t.cpu())
    assert torch.equal(_bits(runs[0]), _bits(runs[1]))
    if kw["mode"] != nat.NORM_DIVIDE and not kw.get("binarize"):
        assert torch.equal(want[2], torch.full((SH.NORM_N,), 5.0 if clip is not None else 7.0))       # the constant window is left as it is


@pytest.mark.parametrize("mode", [nat.NORM_ZSCORE, nat.NORM_DIVIDE])
def test_window_normalize_apply_loop_takes_a_second_trip(ops, mode):
    """the apply pass caps its grid at 16384 blocks of 256: one window of 16384 * 256 + 3 integer values, 513 statistics slots"""
    n = 16384 * 256 + 3
    x = torch.from_numpy(np.random.default_rng(102).integers(0, 256, (1, n)).astype(np.float32))
    g = Guarded(x)
    ops.window_normalize(g.t, mode=mode, divide=255.0)
    _same(g.t, M.window_normalize(x.clone(), mode=mode, divide=255.0), f"window_normalize n={n} mode {mode}")
    assert g.intact()


@pytest.mark.parametrize("mode", [nat.NORM_ZSCORE, nat.NORM_MINMAX])
def test_window_normalize_real_windows_within_the_derived_bound(ops, mode):
    """random real windows: the device adds its fp64 partial sums in another order than numpy, so shift and scale may each be one
    fp32 ulp from the model's, and the result is rounded once: |got - want| <= ulp32(shift) * scale + 2^-22 |want|"""
    n = SH.NORM_N
    x = _randn(3, n, seed=103) * torch.tensor([[1.0], [30.0], [0.01]]) + torch.tensor([[0.0], [100.0], [-3.0]])
    got = ops.window_normalize(x.clone().cuda(), mode=mode).cpu().double()
    want = M.window_normalize(x.clone(), mode=mode).double()
    for b in range(3):
        shift, scale = M.window_coefficients(x[b].numpy(), mode)
        assert float(scale) != 1.0
        bound = float(np.spacing(np.abs(shift))) * float(scale) + 2.0 ** -22 * want[b].abs()
        err = (got[b] - want[b]).abs()
        print(f"window_exact window_normalize real mode {mode} window {b}: max err {float(err.max()):.3g}, max err / bound {float((err / bound).max()):.3g}")
        assert bool((err <= bound).all())


# ---- resample_region -----------------------------------------------------------------------------------------------------------------------
def _box(rng, dt, shape):
    if dt == "float32":
        return (rng.standard_normal(shape) * 100).astype(np.float32)
    if dt == "float64":
        return rng.standard_normal(shape) * 1000 + rng.random(shape) * 1e-7                  # no fp32 holds these exactly
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)                   # uint32 / int32: mostly above 2^24


def _tables(rng, dims, ext, lin, outside, mixed=False):
    i0, i1, f = [], [], []
    for a, n in enumerate(dims):
        lo = rng.integers(0, ext[a] - 1, n).astype(np.int32)
        if lin[a]:
            hi, fr = lo + 1, (rng.random(n) * 0.98 + 0.01).astype(np.float32)                 # i1 != i0, f in (0, 1)
            if mixed:                                                                         # f = 0 on some entries of the axis: the kernel
                fr[rng.choice(n, n // 2, replace=False)] = 0.0                                # picks nearest or trilinear voxel by voxel
        else:
            hi, fr = lo.copy(), np.zeros(n, np.float32)
        if outside:
            lo[rng.choice(n, 2, replace=False)] = -1
        i0.append(lo); i1.append(hi.astype(np.int32)); f.append(fr)
    assert all(int(h.max()) < e for h, e in zip(i1, ext))                                     # every tap lies in the box
    return tuple(torch.from_numpy(np.concatenate(t)) for t in (i0, i1, f))


@pytest.mark.parametrize("dt", sorted(nat.RAW_DTYPES))
def test_resample_region_every_dtype_and_table_arrangement(ops, dt):
    """boxes stored channel last with z / y exchanged; interpolation on all axes, on one, on none, with i0 = -1 entries on each axis, and
    with f = 0 on half the entries of every axis (nearest and trilinear voxels in one launch)"""
    rng = np.random.default_rng(111)
    for dims in ((6, 5, 7), SH.RESAMPLE_SECOND):
        nz, ny, nx = dims
        box = _box(rng, dt, (ny, nz, nx, 2))                                                  # stored (y, z, x, c)
        strides = (1, nx * 2, nz * nx * 2, 2)                                                 # (c, z, y, x) element strides
        raw = torch.from_numpy(box.reshape(-1).view(np.uint8).copy())
        if dt == "uint32":
            assert int((box > 2 ** 24).sum()) > box.size // 2
        for lin, outside, mixed in (((True, True, True), False, False), ((False, True, False), False, False), ((False, False, False), False, False),
                                    ((True, True, True), True, False), ((False, False, True), True, False), ((False, False, False), True, False),
                                    ((True, True, True), False, True), ((True, True, True), True, True)):
            i0, i1, f = _tables(rng, dims, dims, lin, outside, mixed)
            got = ops.resample_region(raw.cuda(), dt, strides, 2, i0.cuda(), i1.cuda(), f.cuda(), dims)
            want = M.resample_region(raw, dt, strides, 2, i0, i1, f, dims)
            _same(got, want, f"resample {dt} {dims} lin {lin} outside {outside} mixed {mixed}")
            if mixed:                                               # both branches inside one launch
                fz, fy, fx = f[:nz], f[nz:nz + ny], f[nz + ny:]
                lin_vox = (fz != 0)[:, None, None] | (fy != 0)[None, :, None] | (fx != 0)[None, None, :]
                assert bool(lin_vox.any()) and not bool(lin_vox.all())
            if outside:
                assert bool((want == 0).all(0).any())


# ---- the activations: the only toleranced checks ---------------------------------------------------------------------------------------------
def _held(what, hip, run):
    """run(dtype) -> the model on the CPU in that dtype: max|hip - f64| <= FACTOR * max|f32cpu - f64| + FLOOR"""
    f64, f32 = run(torch.float64), run(torch.float32).double()
    eh, ec = float((hip.cpu().double() - f64).abs().max()), float((f32 - f64).abs().max())
    print(f"window_exact {what}: max|hip - f64| {eh:.3g}, max|f32cpu - f64| {ec:.3g}, bound {FACTOR * ec + FLOOR:.3g}")
    assert eh <= FACTOR * ec + FLOOR, what


def _act_input(shape, seed):
    x = _randn(*shape, seed=seed) * 4
    flat = x.view(-1)
    k = torch.randperm(flat.numel(), generator=_gen(seed + 1))[:max(4, flat.numel() // 50)]
    flat[k] = torch.tensor([30.0, -30.0])[torch.arange(len(k)) % 2]
    return x


@pytest.mark.parametrize("act", [nat.ACT_SIGMOID, nat.ACT_TANH])
def test_blend_finalize_activations(ops, act):
    for C, n in ((3, 257), (1, 8192 * 256 + 3)):
        v0 = _act_input((C, n), 121)
        w0 = torch.rand(n, generator=_gen(122)) * 1.5 + 0.5
        value = Guarded(v0)
        ops.blend_finalize(value.t, w0.cuda(), clamp=1e-4, act=act)
        assert value.intact()

        def run(dt):
            v = v0.to(dt)
            M.blend_finalize(v, w0, clamp=1e-4, act=act)
            return v
        _held(f"blend_finalize act {act} C={C} n={n}", value.t, run)


@pytest.mark.parametrize("channels_last", [False, True], ids=["planar", "channels_last"])
@pytest.mark.parametrize("act", [nat.ACT_SIGMOID, nat.ACT_TANH, nat.ACT_SOFTMAX])
def test_channel_activation_over_a_sub_range(ops, act, channels_last):
    for C, (c0, c1) in ((3, (1, 3)), (7, (2, 6)), (8, (0, 8)), (8, (3, 4))):
        x = _act_input((6, 8, 11, C) if channels_last else (C, 6, 8, 11), 130 + C)      # 528 voxels: whole float4s for every C
        g = Guarded(x)
        ops.channel_activation(g.t, c0, c1, act, 1.5, channels_last=channels_last)
        assert g.intact()
        keep = [c for c in range(C) if not c0 <= c < c1]
        sel = (lambda t, idx: t[..., idx]) if channels_last else (lambda t, idx: t[idx])
        assert torch.equal(_bits(sel(g.t.cpu(), keep)), _bits(sel(x, keep))), "an untouched channel changed"

        def run(dt):
            v = x.to(dt)
            M.channel_activation(v, c0, c1, act, 1.5, channels_last=channels_last)
            return v
        _held(f"channel_activation act {act} {'channels_last' if channels_last else 'planar'} C={C} [{c0},{c1})", g.t, run)


def _both_forms(ops, x, c0, c1, act, scale):
    a, b = x.clone(), x.clone()
    ops.channel_activation(a, c0, c1, act, scale, channels_last=True)
    ops.set_tuning("channel_act_flat", 0)
    try:
        ops.channel_activation(b, c0, c1, act, scale, channels_last=True)
    finally:
        ops.set_tuning("channel_act_flat", 1)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the flat and the per-voxel form differ"
    return a


@pytest.mark.parametrize("act", [nat.ACT_SIGMOID, nat.ACT_TANH])
@pytest.mark.parametrize("size", ["stride", "ragged"])
def test_flat_and_per_voxel_channel_activation_agree(ops, act, size):
    """the flat float4 form at the size where its stride loop iterates, and a size that is no whole number of float4s (per-voxel form
    whatever the knob says): equal bits on the device, a seeded sample of 10^5 elements against the CPU"""
    nv, C = SH.ACT_FLAT if size == "stride" else SH.ACT_RAGGED
    c0, c1 = 2, 6
    x = torch.randn(nv, C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(141)) * 4
    a = _both_forms(ops, x, c0, c1, act, 1.5)
    n = nv * C
    idx = torch.randint(0, n, (min(n, 100000),), generator=_gen(142))
    idx[:8] = torch.tensor([0, 1, 2, 3, n - 4, n - 3, n - 2, n - 1])
    ch = idx % C
    xs, got = x.view(-1)[idx.cuda()].cpu(), a.view(-1)[idx.cuda()].cpu()
    touched = (ch >= c0) & (ch < c1)
    assert torch.equal(_bits(got[~touched]), _bits(xs[~touched])), "an untouched channel changed"

    def run(dt):
        v = xs[touched].to(dt).view(1, -1).clone()
        M.channel_activation(v, 0, 1, act, 1.5)
        return v.view(-1)
    _held(f"channel_activation flat/per-voxel {size} act {act} ({nv} x {C})", got[touched], run)

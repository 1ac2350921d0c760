"""The decoder joins against fp64 references with NO tolerance (tests/decoder_exact_cases.py): UpCat and the deconv-first placement,
forward and data gradient, in both storage types -- upcat_gemm_kernel<T, FWD | DGRAD> and upcat_copy_channels_kernel; the thin transposed
convs (convT3d_thin_kernel, convT3d_c1_dots_kernel + convT3d_c1_gather_kernel); and RSUNet's bilinear up-sampling pair
(dwconvT3d_generic_kernel, dwconvT3d_generic_vec_kernel, dwconv3d_generic_kernel).

On the operands filed there the fp32 accumulator holds the fp64 sum in any order and the only roundings are the staging of the fp32
weights (and of the folded face sums G') as bf16 MFMA operands and the store, so the kernels must give the reference's BITS.

Every case asserts its premises (decoder_exact_cases.premises, the helper the host proof uses); calls the C entry points as hip_ops
calls them with every output inside a NaN-filled buffer with guard bands and every operand inside a NaN-filled buffer -- bits equal,
every element written, guards intact, and a read past an operand would reach the result; runs a second time through hip_ops and must
repeat; checks the skip half and dx_e against the SOURCE bits and each replicated face against the plane it copies; and, on the fp32
route, the identity <dcat, fwd(x)> = <dx_e, x_e> + <dx_low, x_low> + <db, bias> in exact arithmetic.
tests/test_host_decoder_exact_cases.py proves that the cases discriminate; profiles/decoder_layernorm_exact_seeded_defects.txt records
defects put into the kernels themselves and the cases that went red."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import decoder_exact_cases as X  # noqa: E402
from test_gpu_pw_conv_exact import _bits, _guarded, _guards_intact  # noqa: E402  (the guard-band helpers of the pw-conv suite)

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ops():
    from pytorch_connectomics_amd import _native as nat, hip_ops as ops
    return nat, ops


def _same_bits(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    """bit equality over the whole tensor; on failure the count and the first differing elements"""
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), f"{what}: {got.dtype} {tuple(got.shape)}"
    nan = int(torch.isnan(got.float()).sum())
    assert nan == 0, f"{what}: {nan} of {got.numel()} elements were never written"
    if torch.equal(_bits(got), _bits(want)):
        return
    idx = (got != want).nonzero()
    first = [(tuple(i.tolist()), float(got[tuple(i)]), float(want[tuple(i)])) for i in idx[:8]]
    raise AssertionError(f"{what}: {len(idx)} of {got.numel()} elements differ (exact inputs: none may); last-axis indices "
                         f"{sorted(set(idx[:, -1].tolist()))[:16]}; first (index), got, want: {first}")


class _Dev:
    """the operands of a case on the device, each inside a NaN-filled guarded buffer"""

    def __init__(self, c):
        d = X.operands(c)
        dt = X.TORCH_DT[c.dt]
        self.bufs = {}

        def put(name, a, t):
            if a is None:
                return None
            v, buf = _guarded(a.shape, t, X.to_storage(a, "f32" if t == torch.float32 else "bf16").to(DEV))
            self.bufs[name] = buf
            return v

        self.x, self.xe, self.dcat = put("x", d["x"], dt), put("xe", d["xe"], dt), put("dcat", d["dcat"], dt)
        self.w, self.bias = put("w", d["w"], torch.float32), put("bias", d["bias"], torch.float32)

    def guards_intact(self, what):
        for name, buf in self.bufs.items():
            _guards_intact(buf, f"{what} operand {name}")


def _abi(c, dv):
    """forward and data gradient through the C entry points, as hip_ops calls them, into guarded NaN-filled outputs"""
    nat, ops = _ops()
    lib, p = nat.lib(), ops._p
    dt = X.TORCH_DT[c.dt]
    C_in, C_e, C_u = c.ch
    code, st = ops.dtype_code(dt), ops._stream()
    cat, cat_buf = _guarded((c.N, *c.skip, c.Ct), dt)
    dxl, dxl_buf = _guarded((c.N, *c.low, C_in), dt)
    dxe, dxe_buf = _guarded((c.N, *c.skip, C_e), dt) if C_e else (None, None)
    if c.place == "upcat":
        dims = (c.N, *c.low, *c.skip)
        nat.check(lib.pytc_upcat_deconv2_fwd(p(dv.x), p(dv.w), p(dv.bias), p(dv.xe), p(cat), *dims, C_in, C_e, C_u, code, st), c.id)
        nat.check(lib.pytc_upcat_deconv2_bwd_data(p(dv.dcat), p(dv.w), p(dxe), p(dxl), *dims, C_in, C_e, C_u, code, st), c.id)
    else:
        dims = (c.N, *c.low)
        nat.check(lib.pytc_deconv2_upfirst_fwd(p(dv.x), p(dv.w), p(dv.bias), p(dv.xe), p(cat), *dims, C_in, C_e, C_u, code, st), c.id)
        nat.check(lib.pytc_deconv2_upfirst_bwd_data(p(dv.dcat), p(dv.w), p(dxe), p(dxl), *dims, C_in, C_e, C_u, code, st), c.id)
    torch.cuda.synchronize()
    for buf, name in ((cat_buf, "cat"), (dxl_buf, "dx_low"), (dxe_buf, "dx_e")):
        if buf is not None:
            _guards_intact(buf, f"{c.id} {name}")
    return cat, dxe, dxl


def _through_ops(c, dv):
    _, ops = _ops()
    C_e = c.ch[1]
    if c.place == "upcat":
        cat = ops.upcat_deconv2_fwd(dv.x, dv.w, dv.bias, dv.xe)
        dxe, dxl, _, db = ops.upcat_deconv2_bwd(dv.dcat, dv.x, dv.w, C_e, want_w=False, want_b=True)
    else:
        cat = ops.deconv2_upfirst_fwd(dv.x, dv.w, dv.xe, dv.bias)
        dxe, dxl, _, db = ops.deconv2_upfirst_bwd(dv.dcat, dv.x, dv.w, C_e, want_w=False, want_b=True)
    torch.cuda.synchronize()
    return cat, dxe, dxl, db


def _run_case(c):
    ref = X.premises(c)
    C_in, C_e, C_u = c.ch
    dv = _Dev(c)
    cat, dxe, dxl = _abi(c, dv)
    _same_bits(cat, X.to_storage(ref["cat"], c.dt), f"{c.id} cat")
    _same_bits(dxl, X.to_storage(ref["dx_low"], c.dt), f"{c.id} dx_low")
    if C_e:
        _same_bits(dxe, X.to_storage(ref["dx_e"], c.dt), f"{c.id} dx_e")
        # the two copies move bits: against the source tensors themselves
        assert torch.equal(_bits(cat[..., c.skip_off:c.skip_off + C_e]), _bits(dv.xe)), f"{c.id}: the skip half is not the skip"
        assert torch.equal(_bits(dxe), _bits(dv.dcat[..., c.skip_off:c.skip_off + C_e])), f"{c.id}: dx_e is not dcat's skip half"
    up = cat[..., c.up_off:c.up_off + C_u]
    for axis in range(3):
        if c.odd[axis]:
            a = up.movedim(1 + axis, 0)
            assert torch.equal(_bits(a[2 * c.low[axis]]), _bits(a[2 * c.low[axis] - 1])), f"{c.id}: face of axis {axis} is not plane 2d - 1"
    # a second launch, through hip_ops, repeats the bits
    cat2, dxe2, dxl2, db = _through_ops(c, dv)
    assert torch.equal(_bits(cat2), _bits(cat)) and torch.equal(_bits(dxl2), _bits(dxl)), f"{c.id}: hip_ops / a second run differs"
    if C_e:
        assert torch.equal(_bits(dxe2), _bits(dxe)), f"{c.id}: dx_e through hip_ops differs"
    dv.guards_intact(c.id)
    if c.dt == "f32":
        # every factor is a multiple of 1/4 below 2^9 and every sum has fewer than 2^20 terms: exact in fp64 in any order
        f = lambda t: t.double()
        lhs = (f(dv.dcat) * f(cat)).sum()
        rhs = (f(dxl) * f(dv.x)).sum() + ((f(dxe) * f(dv.xe)).sum() if C_e else 0.0)
        if dv.bias is not None:
            rhs = rhs + (f(db) * f(dv.bias)).sum()
        assert float(lhs) == float(rhs), f"{c.id}: <dcat, fwd(x)> = {float(lhs)} but <bwd(dcat), x> = {float(rhs)}"


@pytest.mark.parametrize("c", X.upcat_cases(), ids=X.ids(X.upcat_cases()))
def test_upcat_forward_and_data_gradient_exact(c):
    _run_case(c)


@pytest.mark.parametrize("c", X.upfirst_cases(), ids=X.ids(X.upfirst_cases()))
def test_deconv_first_forward_and_data_gradient_exact(c):
    _run_case(c)


@pytest.mark.parametrize("c", X.special_cases(), ids=X.ids(X.special_cases()))
def test_roundings_and_copy_cap_exact(c):
    _run_case(c)


def test_more_row_tiles_than_one_launch_takes_are_refused_by_name():
    """65535 x 64 + 1 low-resolution rows (C_in 8, C_e 1, C_u 1, bf16): the row tiles sit on gridDim.y, so the entry points refuse with
    the limit in the message before anything is launched or written (buffers are allocated, never initialised or read)."""
    _, ops = _ops()
    rows = X.MAX_ROW_TILES * X.UP_BQ + 1
    assert X.refused_rows(rows) and not X.refused_rows(rows - 1)
    bf = torch.bfloat16
    x = torch.empty((1, 1, 1, rows, 8), dtype=bf, device=DEV)
    w = torch.zeros((8, 1, 2, 2, 2), dtype=torch.float32, device=DEV)
    xe = torch.empty((1, 2, 2, 2 * rows, 1), dtype=bf, device=DEV)
    dcat = torch.empty((1, 2, 2, 2 * rows, 2), dtype=bf, device=DEV)
    calls = {
        "upcat_deconv2_fwd": lambda: ops.upcat_deconv2_fwd(x, w, None, xe),
        "upcat_deconv2_bwd_data": lambda: ops.upcat_deconv2_bwd(dcat, x, w, 1, want_w=False, want_b=False),
        "deconv2_upfirst_fwd": lambda: ops.deconv2_upfirst_fwd(x, w, xe),
        "deconv2_upfirst_bwd_data": lambda: ops.deconv2_upfirst_bwd(dcat, x, w, 1, want_w=False, want_b=False),
    }
    for name, call in calls.items():
        with pytest.raises(RuntimeError) as err:
            call()
        msg = str(err.value)
        assert name in msg and str(X.MAX_ROW_TILES) in msg and str(rows) in msg, f"{name}: {msg!r}"
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- B. thin transposed convs
def _guarded_operand(a: np.ndarray, t):
    v, buf = _guarded(a.shape, t, X.to_storage(a, "f32" if t == torch.float32 else "bf16").to(DEV))
    return v, buf


def _thin_entry(c, x, w, bias):
    """pytc_convT3d_thin_fwd itself (hip_ops sends C_out = 1 to the dots + gather pair), into a guarded NaN-filled output"""
    nat, ops = _ops()
    y, ybuf = _guarded((c.N, *c.out_grid, c.cout), X.TORCH_DT[c.dt])
    nat.check(nat.lib().pytc_convT3d_thin_fwd(ops._p(x), ops._p(w), ops._p(bias), ops._p(y), c.N, ops._i3(c.grid), c.cin, c.cout,
                                             ops.dtype_code(y.dtype), ops._stream()), c.id)
    torch.cuda.synchronize()
    _guards_intact(ybuf, f"{c.id} thin entry")
    return y


def _thin_operands(c):
    d = X.thin_operands(c)
    x, xbuf = _guarded_operand(d["x"], X.TORCH_DT[c.dt])
    w, wbuf = _guarded_operand(d["w"], torch.float32)
    bias, bbuf = _guarded_operand(d["bias"], torch.float32) if d["bias"] is not None else (None, None)
    return x, w, bias, [b for b in (xbuf, wbuf, bbuf) if b is not None]


@pytest.mark.parametrize("c", X.thin_cases(), ids=X.ids(X.thin_cases()))
def test_thin_transposed_conv_exact_on_both_routes(c):
    nat, ops = _ops()
    want = X.to_storage(X.thin_premises(c)["y"], c.dt)
    assert ops.convT3d_thin_supported(c.cin, c.cout) and X.thin_supported(c.cin, c.cout)
    x, w, bias, bufs = _thin_operands(c)
    direct = _thin_entry(c, x, w, bias)
    _same_bits(direct, want, f"{c.id} [convT3d_thin_kernel]")
    routed = ops.convT3d_thin(x, w, bias)                      # C_out = 1: convT3d_c1_dots_kernel + convT3d_c1_gather_kernel
    torch.cuda.synchronize()
    _same_bits(routed, want, f"{c.id} [hip_ops route: {X.thin_routes(c.cin, c.cout)[0]}]")
    _same_bits(_thin_entry(c, x, w, bias), direct, f"{c.id}: a second run")
    for b in bufs:
        _guards_intact(b, f"{c.id} operand")


def test_thin_supported_is_the_restated_rule():
    _, ops = _ops()
    for ci, co in ((144, 4), (600, 1), (512, 1), (152, 4), (608, 1), (12, 1), (8, 5), (8, 1), (16, 0), (0, 1)):
        assert ops.convT3d_thin_supported(ci, co) == X.thin_supported(ci, co), (ci, co)


def test_thin_grid_stride_second_trip_exact():
    """17 039 360 outputs against 65 536 x 256 threads: the expected tensor is the one-channel closed form, compared on the device"""
    c = X.thin_cap_case()
    want = X.to_storage(X.thin_premises(c)["y"], c.dt).to(DEV)
    x, w, bias, bufs = _thin_operands(c)
    y = _thin_entry(c, x, w, bias)
    assert not torch.isnan(y.float()).any(), f"{c.id}: outputs were never written"
    bad = int((_bits(y) != _bits(want)).sum())
    assert bad == 0, f"{c.id}: {bad} of {y.numel()} outputs differ"
    assert torch.equal(_bits(_thin_entry(c, x, w, bias)), _bits(y)), f"{c.id}: a second run differs"
    for b in bufs:
        _guards_intact(b, f"{c.id} operand")


# ------------------------------------------------------------------------------------------------------------- C. bilinear up-sampling
def _dw_entries(c, x, dy, taps):
    """the two C entry points, as hip_ops calls them, into guarded NaN-filled outputs -> (y, dx)"""
    nat, ops = _ops()
    k, s, p, _, og = X.dw_geometry(c)
    dt = X.TORCH_DT[c.dt]
    y, ybuf = _guarded((c.N, *og, c.C), dt)
    dx, dxbuf = _guarded((c.N, *c.grid, c.C), dt)
    lib, P, i3 = nat.lib(), ops._p, ops._i3
    nat.check(lib.pytc_dwconvT3d_generic_fwd(P(x), P(y), P(taps), c.N, *c.grid, c.C, i3(k), i3(s), i3(p), ops.dtype_code(dt),
                                             ops._stream()), c.id)
    nat.check(lib.pytc_dwconv3d_generic_fwd(P(dy), P(dx), P(taps), c.N, *og, c.C, i3(k), i3(s), i3(p), i3(c.grid), ops.dtype_code(dt),
                                            ops._stream()), c.id)
    torch.cuda.synchronize()
    _guards_intact(ybuf, f"{c.id} y")
    _guards_intact(dxbuf, f"{c.id} dx")
    return y, dx


@pytest.mark.parametrize("c", X.dw_cases(), ids=X.ids(X.dw_cases()))
def test_bilinear_upsampling_pair_exact(c):
    _, ops = _ops()
    ref = X.dw_premises(c)
    k, s, p, taps64, og = X.dw_geometry(c)
    d = X.dw_operands(c)
    dt = X.TORCH_DT[c.dt]
    x, xbuf = _guarded_operand(d["x"], dt)
    dy, dybuf = _guarded_operand(d["dy"], dt)
    taps, tbuf = _guarded_operand(taps64, torch.float32)
    y, dx = _dw_entries(c, x, dy, taps)
    form = "dwconvT3d_generic_vec_kernel" if X.dw_vectorised(c.C, c.dt) else "dwconvT3d_generic_kernel"
    _same_bits(y, X.to_storage(ref["y"], c.dt), f"{c.id} forward [{form}]")
    _same_bits(dx, X.to_storage(ref["dx"], c.dt), f"{c.id} backward [dwconv3d_generic_kernel]")
    y2 = ops.dwconvT3d_generic(x, taps, k, s, p)
    dx2 = ops.dwconv3d_generic(dy, taps, k, s, p, c.grid)
    torch.cuda.synchronize()
    assert torch.equal(_bits(y2), _bits(y)) and torch.equal(_bits(dx2), _bits(dx)), f"{c.id}: hip_ops / a second run differs"
    # the pair is adjoint, in integers
    lhs, rhs = float((dy.double() * y.double()).sum()), float((dx.double() * x.double()).sum())
    assert lhs == rhs, f"{c.id}: <dy, up(x)> = {lhs} but <down(dy), x> = {rhs}"
    for b in (xbuf, dybuf, tbuf):
        _guards_intact(b, f"{c.id} operand")

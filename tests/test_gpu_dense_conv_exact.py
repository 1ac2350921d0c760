"""The dense-conv kernels against fp64 references with NO tolerance (tests/dense_conv_exact_cases.py): integer / quarter operands make
every partial sum exact in fp32 in any order, so the LDS-tiled matrix-core kernel at MT = 4 / 2 / 1, its eight-phase launch
(ops.convT3d_phase), the data-gradient and padded weight images, the one-input-channel stencil, the thin-input kernel, the MFMA gather
kernel and conv3d_strided must each reproduce the reference bit for bit, over every output element, on a dense data set (accumulation,
pre-activation, padding of f(X), bias, residual, the single rounding of the store) and on an impulse set (every output is one weight or
zero: tap, channel, voxel and output-channel mapping of the kernel and of the weight pack).

Tile and phase cases call the C ABI the way ops.conv3d / ops.convT3d_phase do, with the output a view inside a larger NaN-filled
buffer: an element the kernel does not write stays NaN and fails the comparison, a write past either end of the tensor changes a guard
word.  They run twice and must repeat bit for bit.  The host test (test_host_dense_conv_exact_cases.py) proves the exactness premises
and that each case takes the kernel form and MT it is filed under.

What these cases cannot see: the zero-padded slots of the last K group are guarded twice, by the zero operand the kernel reads for them
(koff = -1) and by the zero weights the pack writes there.  A kernel that read voxel data for those slots would still multiply it by
zero, so with finite inputs its output is the same; measured: that change leaves all cases green, while dropping the second pass's
channel offset turns every MT = 4 case with C_out % 8 == 0 red and swapping the odd-phase tap map every phase case.

A mismatch message names the first differing elements as (n, z, y, x, channel): tile = (z // 4, y // 8, x // 16), seam sides are
z 3 | 4, y 7 | 8, x 15 | 16, phase = parity of (z, y, x) on the 2x grid, channel // 16 = output tile, (channel // 32) % 2 = pass of MT = 4."""
import ctypes as C
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import dense_conv_exact_cases as X  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096          # elements either side of the output tensor


def _ops():
    from pytorch_connectomics_amd import _native as nat, hip_ops as ops
    return nat, ops


def _ids(cs):
    return [c.id for c in cs]


def _check(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    """torch.equal over the whole (N, D, H, W, C) tensor; on failure the count and the first differing elements"""
    got = got.cpu()
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), f"{what}: {got.dtype} {tuple(got.shape)}"
    if torch.equal(got, want):
        return
    bad = (got != want) | got.isnan()
    idx = bad.nonzero()
    first = [(tuple(i.tolist()), float(got[tuple(i)]), float(want[tuple(i)])) for i in idx[:8]]
    raise AssertionError(f"{what}: {len(idx)} of {got.numel()} elements differ (exact inputs: none may); channels "
                         f"{sorted(set(idx[:, 4].tolist()))[:16]}; first (n, z, y, x, c), got, want: {first}")


def _pack(c, w64: torch.Tensor) -> torch.Tensor:
    _, ops = _ops()
    w = w64.float().contiguous().to(DEV)
    if c.layout == "fwd":
        return ops.conv3d_pack_weight(w, c.dtype)
    if c.layout == "dgrad":
        return ops.conv3d_pack_weight_dgrad(w, c.dtype)
    if c.layout == "dgrad_padded":
        assert (c.cout, c.cin) == (ops.pad_channels(c.real[1], c.dtype), ops.pad_channels(c.real[0], c.dtype))
        return ops.conv3d_pack_weight_padded(w, "dgrad", c.dtype, (c.cout, c.cin))
    if c.phase:
        return ops.ConvPackSet().get(w, c.layout, c.dtype)
    return ops.conv3d_pack_weight_direct(w, c.dtype, layout=c.layout)


def _operands(c, d):
    x = X.channels_last(d["x"]).to(c.dtype).to(DEV)
    ab = d["ab"].float().contiguous().to(DEV) if d["ab"] is not None else None
    bias = d["bias"].float().to(DEV) if d["bias"] is not None else None
    res = X.channels_last(d["res"]).to(c.dtype).to(DEV) if d["res"] is not None else None
    return x, ab, bias, res


def _act(d):
    nat, _ = _ops()
    return {"none": (nat.ACT_NONE, 0.0), "relu": (nat.ACT_RELU, 0.0), "leaky": (nat.ACT_LEAKY, X.LEAKY)}[d["act"]]


def _abi_call(c, d, wp):
    """pytc_conv3d_fwd / pytc_convT3d_phase_fwd as ops.conv3d / ops.convT3d_phase call them, the output inside a NaN-filled buffer.
    -> (output view (N, *out_dims, cout), buffer)"""
    nat, _ = _ops()
    x, ab, bias, res = _operands(c, d)
    shape = (c.N,) + c.out_dims + (c.cout,)
    numel = 1
    for v in shape:
        numel *= v
    buf = torch.full((numel + 2 * GUARD,), float("nan"), dtype=c.dtype, device=DEV)
    y = buf[GUARD:GUARD + numel].view(shape)
    a = nat.Conv3dArgs()
    a.x, a.w_packed, a.y = x.data_ptr(), wp.data_ptr(), y.data_ptr()
    a.bias = bias.data_ptr() if bias is not None else None
    a.ab = ab.data_ptr() if ab is not None else None
    a.res = res.data_ptr() if res is not None else None
    a.N, a.C_in, a.C_out = c.N, c.cin, c.cout
    a.D, a.H, a.W = c.out_dims
    a.kd, a.kh, a.kw = c.kernel
    a.act_in, a.act_param = _act(d)
    a.res_mode = nat.RES_ADD if res is not None else nat.RES_NONE
    a.dtype = nat.BF16 if c.dtype == X.BF16 else nat.F32
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if c.phase:
        nat.check(nat.lib().pytc_convT3d_phase_fwd(C.byref(a), (C.c_int32 * 3)(*c.dims), stream), "convT3d_phase")
    else:
        nat.check(nat.lib().pytc_conv3d_fwd(C.byref(a), stream), "conv3d")
    torch.cuda.synchronize()
    return y, buf


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _guarded_exact(c, d, what):
    """the tile / phase check: exact result, guards untouched, every element written, a second run bit-identical"""
    want = X.channels_last(X.reference(c, d))
    wp = _pack(c, d["w"])
    y, buf = _abi_call(c, d, wp)
    fresh = torch.full((GUARD,), float("nan"), dtype=c.dtype, device=DEV)
    assert torch.equal(_bits(buf[:GUARD]), _bits(fresh)), f"{what}: wrote BEFORE the output tensor"
    assert torch.equal(_bits(buf[-GUARD:]), _bits(fresh)), f"{what}: wrote PAST the output tensor"
    _check(y, want, what)                                       # (a NaN left in place is an element the kernel did not write)
    y2, _ = _abi_call(c, d, wp)
    assert torch.equal(_bits(y2), _bits(y)), f"{what}: a second run differs from the first"


def _ops_exact(c, d, what):
    """the other forms through hip_ops"""
    _, ops = _ops()
    want = X.channels_last(X.reference(c, d))
    wp = _pack(c, d["w"])
    x, ab, bias, res = _operands(c, d)
    act, prm = _act(d)
    if c.form == X.STRIDED:
        y = ops.conv3d_strided(x, wp, c_out=c.cout, kernel=c.kernel, stride=c.stride, pad=(1, 1, 1), out_dims=c.out_dims,
                               transposed=c.layout in ("convT", "conv_dgrad"), bias=bias, ab=ab, act_in=act, act_param=prm, res=res)
    else:
        y = ops.conv3d(x, wp, c_out=c.cout, kernel=c.kernel, bias=bias, ab=ab, act_in=act, act_param=prm, res=res)
    torch.cuda.synchronize()
    _check(y, want, what)


def _both_sets(c, check):
    for combo in c.operands:
        check(c, X.dense_data(c, combo), f"{c.id} dense {combo}")
    check(c, X.impulse_data(c), f"{c.id} impulse")


@pytest.mark.parametrize("c", X.cases("tile"), ids=_ids(X.cases("tile")))
def test_tile_form_exact(c):
    assert X.launch_plan(c)[:2] == (X.TILED, c.mt)
    _both_sets(c, _guarded_exact)


@pytest.mark.parametrize("c", X.cases("dgrad"), ids=_ids(X.cases("dgrad")))
def test_tile_form_data_gradient_images_exact(c):
    assert X.launch_plan(c)[:2] == (X.TILED, c.mt)
    _both_sets(c, _guarded_exact)


@pytest.mark.parametrize("c", X.cases("phase"), ids=_ids(X.cases("phase")))
def test_phase_form_exact(c):
    assert X.launch_plan(c)[:2] == (X.TILED, c.mt)
    _both_sets(c, _guarded_exact)


@pytest.mark.parametrize("c", X.cases("stencil"), ids=_ids(X.cases("stencil")))
def test_one_channel_stencil_exact(c):
    _both_sets(c, _ops_exact)


@pytest.mark.parametrize("c", X.cases("thin"), ids=_ids(X.cases("thin")))
def test_thin_input_kernel_exact(c):
    _both_sets(c, _ops_exact)


@pytest.mark.parametrize("c", X.cases("gather"), ids=_ids(X.cases("gather")))
def test_gather_kernel_exact(c):
    assert X.launch_plan(c)[:2] == (X.GATHER, c.mt)
    _both_sets(c, _ops_exact)


@pytest.mark.parametrize("c", X.cases("strided"), ids=_ids(X.cases("strided")))
def test_strided_conv_layouts_exact(c):
    _both_sets(c, _ops_exact)

"""The storage-dtype dispatch of the C ABI (PYTC_DISPATCH_DTYPE / PYTC_CHECK_DTYPE, csrc/pytc_common.h), entry by entry through
_native.lib(): a dtype code that is neither PYTC_F32 nor PYTC_BF16 is refused with PYTC_ERR_INVALID and "<what>: bad dtype <code>"
before anything is launched -- it is never run as the float kernel -- and both valid codes are accepted.

One or two entries per converted source file, each at the smallest shape it takes.  Every device buffer is allocated as fp32 at
that shape, so the float kernel a missed conversion would run stays in bounds and the bf16 run uses half of each buffer.  Outputs
are filled with a sentinel whose bits must survive the refused call."""
import ctypes as C

import pytest
import torch

from pytorch_connectomics_amd import _native as nat

pytestmark = pytest.mark.gpu

BAD = 7
SENTINEL = -12345.678


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _i3(v):
    return (C.c_int32 * 3)(*v)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _in(*shape):
    g = torch.Generator().manual_seed(sum(shape) + len(shape))
    return torch.randn(shape, generator=g, dtype=torch.float32).cuda()


def _out(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")


# Each case: name -> (what, build), build(lib) -> (call(dtype) -> status, [output tensors]).  `what` is the prefix of the refusal.
def _layernorm_rows(lib):
    x, g, b, y = _in(4, 16), _in(16), _in(16), _out(4, 16)
    return (lambda dt: lib.pytc_layernorm_rows(_p(x), _p(y), _p(g), _p(b), 4, 16, 1e-5, dt, _stream())), [y]


def _affine_act(lib):
    x, ab, y = _in(1, 4, 16), _in(1, 2, 16), _out(1, 4, 16)
    return (lambda dt: lib.pytc_affine_act(_p(x), _p(y), _p(ab), 1, 4, 16, nat.ACT_RELU, 0.0, dt, _stream())), [y]


def _layernorm_rows_bwd(lib):
    dy, x, g, dx = _in(4, 16), _in(4, 16), _in(16), _out(4, 16)
    partial = _out(lib.pytc_layernorm_rows_bwd_slots(4, 16, nat.F32), 2, 16)
    return (lambda dt: lib.pytc_layernorm_rows_bwd(_p(dy), _p(x), _p(g), _p(dx), _p(partial), 4, 16, 1e-5, dt, _stream())), [dx, partial]


def _layernorm_any(lib):
    x, g, b, y = _in(4, 16), _in(16), _in(16), _out(4, 16)
    return (lambda dt: lib.pytc_layernorm_any(_p(x), _p(y), _p(g), _p(b), 4, 16, 1e-5, dt, _stream())), [y]


def _linear_fwd(lib):
    x, w, b, y = _in(4, 16), _in(16, 16), _in(16), _out(4, 16)
    return (lambda dt: lib.pytc_linear_fwd(_p(x), _p(w), _p(b), None, 0, None, _p(y), 4, 16, 16, 0, dt, _stream())), [y]


def _upcat_dims():
    return 1, 2, 2, 2, 4, 4, 4, 16, 16, 16          # N, low grid, skip grid, C_in, C_e, C_u


def _upcat_deconv2_fwd(lib):
    N, d, h, w, D, H, W, ci, ce, cu = _upcat_dims()
    x_low, wt, b, x_e, cat = _in(N, d, h, w, ci), _in(ci, cu, 2, 2, 2), _in(cu), _in(N, D, H, W, ce), _out(N, D, H, W, ce + cu)
    return (lambda dt: lib.pytc_upcat_deconv2_fwd(_p(x_low), _p(wt), _p(b), _p(x_e), _p(cat), N, d, h, w, D, H, W, ci, ce, cu, dt,
                                                  _stream())), [cat]


def _upcat_deconv2_wgrad(lib):
    N, d, h, w, D, H, W, ci, ce, cu = _upcat_dims()
    rows = N * d * h * w
    x_low, dcat = _in(N, d, h, w, ci), _in(N, D, H, W, ce + cu)
    ws = _out(max(int(lib.pytc_upcat_deconv2_wgrad_ws_elems(rows, ci, cu, dt)) for dt in (nat.F32, nat.BF16)))
    dw, db = _out(ci, cu, 2, 2, 2), _out(cu)
    return (lambda dt: lib.pytc_upcat_deconv2_wgrad(_p(x_low), _p(dcat), _p(ws), _p(dw), _p(db), N, d, h, w, D, H, W, ci, ce, cu, dt,
                                                    _stream())), [ws, dw, db]


def _deconv2_upfirst_fwd(lib):
    N, d, h, w, D, H, W, ci, ce, cu = _upcat_dims()
    x_low, wt, b, x_e, out = _in(N, d, h, w, ci), _in(ci, cu, 2, 2, 2), _in(cu), _in(N, D, H, W, ce), _out(N, D, H, W, ce + cu)
    return (lambda dt: lib.pytc_deconv2_upfirst_fwd(_p(x_low), _p(wt), _p(b), _p(x_e), _p(out), N, d, h, w, ci, ce, cu, dt, _stream())), [out]


def _gelu(lib):
    x, y = _in(64), _out(64)
    return (lambda dt: lib.pytc_gelu(_p(x), None, _p(y), 64, dt, _stream())), [y]


def _copy_zero_front(lib):
    x, y = _in(1, 2, 2, 2, 16), _out(1, 2, 2, 2, 16)
    return (lambda dt: lib.pytc_copy_zero_front(_p(x), _p(y), 1, _i3((2, 2, 2)), 16, dt, _stream())), [y]


def _dw_wgrad(lib):
    # K = 5: neither the z-march nor the 16-byte vector form, the generic kernel with 8-byte (fp32: 2-wide) channel vectors
    dims, Cc, K = _i3((2, 2, 2)), 4, 5
    g, x = _in(1, 2, 2, 2, Cc), _in(1, 2, 2, 2, Cc)
    slots = max(lib.pytc_dw_wgrad_slots(1, dims, dims, Cc, K, 1, dt) for dt in (nat.F32, nat.BF16))
    assert slots >= 1
    ws, dW, db = _out(slots * (K ** 3 * Cc + Cc)), _out(K ** 3, Cc), _out(Cc)
    return (lambda dt: lib.pytc_dw_wgrad(_p(g), _p(x), _p(dW), _p(db), _p(ws), 1, dims, dims, Cc, K, 1, dt, _stream())), [ws, dW, db]


def _maxpool3d_bwd(lib):
    x, dy, dx = _in(1, 2, 2, 2, 16), _in(1, 1, 1, 1, 16), _out(1, 2, 2, 2, 16)
    return (lambda dt: lib.pytc_maxpool3d_bwd(_p(x), _p(dy), _p(dx), 1, 2, 2, 2, 16, 2, 2, 2, dt, _stream())), [dx]


def _act_bwd(lib):
    da, x, dt_ = _in(1, 4, 16), _in(1, 4, 16), _out(1, 4, 16)
    return (lambda dt: lib.pytc_act_bwd(_p(da), _p(x), None, _p(dt_), None, 1, 4, 16, nat.ACT_RELU, 0.0, dt, _stream())), [dt_]


def _dwconv3d_fwd(lib):
    x, w, b, y = _in(1, 2, 2, 2, 16), _in(27, 16), _in(16), _out(1, 2, 2, 2, 16)
    return (lambda dt: lib.pytc_dwconv3d_fwd(_p(x), _p(y), _p(w), _p(b), None, 1, 2, 2, 2, 16, 3, 1, dt, _stream())), [y]


def _pw_pack_weight(lib):
    w = _in(16, 16)
    packed = _out(max(int(lib.pytc_pw_packed_elems(16, 16, dt)) for dt in (nat.F32, nat.BF16)))
    return (lambda dt: lib.pytc_pw_pack_weight(_p(w), 16, 16, 0, _p(packed), dt, _stream())), [packed]


def _conv3d_pack_weight(lib):
    w = _in(16, 16, 3, 3, 3)
    packed = _out(max(int(lib.pytc_conv3d_packed_elems(16, 16, 3, 3, 3, dt)) for dt in (nat.F32, nat.BF16)))
    return (lambda dt: lib.pytc_conv3d_pack_weight(_p(w), 16, 16, 3, 3, 3, _p(packed), dt, _stream())), [packed]


def _conv3d_pack_weight_direct(lib):
    w = _in(16, 16, 3, 3, 3)
    packed = _out(max(int(lib.pytc_conv3d_direct_packed_elems(16, 16, 3, 3, 3, dt)) for dt in (nat.F32, nat.BF16)))
    return (lambda dt: lib.pytc_conv3d_pack_weight_direct(_p(w), 16, 16, 3, 3, 3, 16 * 27, 27, 0, _p(packed), dt, _stream())), [packed]


def _convT3d_thin(lib):
    x, w, b, y = _in(1, 2, 2, 2, 8), _in(8, 2, 3, 3, 3), _in(2), _out(1, 4, 4, 4, 2)
    return (lambda dt: lib.pytc_convT3d_thin_fwd(_p(x), _p(w), _p(b), _p(y), 1, _i3((2, 2, 2)), 8, 2, dt, _stream())), [y]


def _gather_windows(lib):
    vol, out = _in(2, 4, 4, 4), _out(1, 2, 2, 2, 2)
    return (lambda dt: lib.pytc_gather_windows(_p(vol), 2, 4, 4, 4, _i3((1, 1, 1)), 1, 2, 2, 2, 0, nat.PAD_CONSTANT, 0.0, _p(out), dt,
                                               _stream())), [out]


def _blend_accumulate(lib):
    pred, wz, value, weight = _in(1, 2, 2, 2, 2), torch.ones(2, device="cuda"), _out(2, 4, 4, 4), _out(4, 4, 4)
    return (lambda dt: lib.pytc_blend_accumulate(_p(pred), dt, 1, _i3((1, 1, 1)), 2, 2, 2, 2, 0, _p(wz), _p(wz), _p(wz),
                                                 nat.BLEND_PRODUCT, 0.0, None, _p(value), _p(weight), 4, 4, 4, _stream())), [value, weight]


# pw_gemm_kernels.hip takes bf16 only and has no dispatch; its launch goes through pytc_pw_conv_fwd (pw_kernels.hip)
CASES = {
    "layernorm_rows": ("layernorm_rows", _layernorm_rows),                              # norm_pool_kernels.hip
    "affine_act": ("affine_act", _affine_act),
    "layernorm_rows_bwd": ("layernorm_rows_bwd", _layernorm_rows_bwd),                  # norm_variant_kernels.hip
    "layernorm_any": ("layernorm_any", _layernorm_any),                                 # swin_kernels.hip
    "linear_fwd": ("linear_fwd", _linear_fwd),                                          # transformer_kernels.hip
    "upcat_deconv2_fwd": ("upcat_deconv2_fwd", _upcat_deconv2_fwd),                     # upcat_kernels.hip
    "upcat_deconv2_wgrad": ("upcat_deconv2_wgrad", _upcat_deconv2_wgrad),
    "deconv2_upfirst_fwd": ("deconv2_upfirst_fwd", _deconv2_upfirst_fwd),
    "gelu": ("gelu", _gelu),                                                            # train_kernels.hip
    "copy_zero_front": ("copy_zero_front", _copy_zero_front),                           # (ran as 4-byte elements on a bad code)
    "dw_wgrad": ("dw_wgrad", _dw_wgrad),                                                # (ran the float kernel on a bad code)
    "maxpool3d_bwd": ("maxpool3d_bwd", _maxpool3d_bwd),                                 # rsunet_train_kernels.hip (cleared dx first)
    "act_bwd": ("act_bwd", _act_bwd),
    "dwconv3d_fwd": ("dwconv3d", _dwconv3d_fwd),                                        # dwconv_kernels.hip
    "pw_pack_weight": ("pw_pack_weight", _pw_pack_weight),                              # pw_kernels.hip
    "conv3d_pack_weight": ("conv3d_pack_weight", _conv3d_pack_weight),                  # conv3d_kernels.hip
    "conv3d_pack_weight_direct": ("conv3d_pack_weight_direct", _conv3d_pack_weight_direct),     # conv3d_strided_kernels.hip
    "convT3d_thin_fwd": ("convT3d_thin", _convT3d_thin),
    "gather_windows": ("gather_windows", _gather_windows),                              # window_kernels.hip
    "blend_accumulate": ("blend_accumulate", _blend_accumulate),
}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return nat.lib()


@pytest.mark.parametrize("name", sorted(CASES))
def test_bad_dtype_is_refused_before_any_launch(lib, name):
    what, build = CASES[name]
    call, outs = build(lib)
    before = [o.clone() for o in outs]
    torch.cuda.synchronize()
    status = call(BAD)
    torch.cuda.synchronize()
    assert status == nat.ERR_INVALID
    assert lib.pytc_last_error().decode() == f"{what}: bad dtype {BAD}"
    for o, b in zip(outs, before):
        assert torch.equal(o.view(torch.int32), b.view(torch.int32)), "a refused call wrote to an output"


@pytest.mark.parametrize("dtype", ["F32", "BF16"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_valid_dtype_is_accepted(lib, name, dtype):
    call, _ = CASES[name][1](lib)
    status = call(getattr(nat, dtype))
    torch.cuda.synchronize()
    assert status == nat.OK, lib.pytc_last_error().decode()

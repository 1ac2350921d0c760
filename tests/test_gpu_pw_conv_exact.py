"""The single pointwise convolution pytc_pw_conv_fwd in every launch form against fp64 references with NO tolerance
(tests/pw_conv_exact_cases.py): on the operands filed there every product and every partial sum is an fp32 number in any order, GELU is
met only where the device functions are exact, and the only roundings are the conversion of an fp32 value into a bf16 MFMA operand and
the store -- so pw_conv_kernel (four dtype routes, MT 1 / 2 / 4), pw_stem_kernel, pw_head_kernel, the six pw_fast_kernel instances with
their blockIdx.z shares, and the four pw_gemm_lds_kernel<false, BR, KS, true> instances must give the reference's BITS.

Every case asserts its premises (pw_conv_exact_cases.assert_premises, the helper the host proof uses) and what the library reports
about its dispatch (pytc_pw_conv_paired_supported, pytc_pw_conv_rowmajor_supported against the restated rules); writes into a NaN-filled
buffer with guard bands -- bits equal, every element written, guards intact -- runs twice and must repeat; and where the same operands
can run on another kernel (pw_thin = 0, or the unpaired weight image on the generic kernel, or the paired image for the row-major form)
that kernel must give the same bits.  The packers are compared whole against numpy restatements of their layouts, and every call the
header forbids must return an error and leave its output untouched.  tests/test_host_pw_conv_exact_cases.py proves that the cases
discriminate; profiles/pw_conv_exact_seeded_defects.txt records five defects put into the kernels themselves and the cases that went
red.  The whole file takes about 3 s on an MI355X, the slowest case 0.35 s."""
import contextlib
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import pw_conv_exact_cases as X  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096          # elements either side of every guarded tensor
bf = torch.bfloat16


def _ops():
    from pytorch_connectomics_amd import _native as nat, hip_ops as ops
    return nat, ops


@contextlib.contextmanager
def _knobs(**knobs):
    _, ops = _ops()
    try:
        for k, v in knobs.items():
            ops.set_tuning(k, v)
        yield
    finally:
        for k, v in X.KNOB_DEFAULTS.items():
            ops.set_tuning(k, v)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _guarded(shape, dtype, fill=None, value=float("nan")):
    """(view of `shape`, whole buffer): the view sits GUARD elements inside a buffer filled with `value`"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), value, dtype=dtype, device=DEV)
    v = buf[GUARD:GUARD + n].view(tuple(shape))
    if fill is not None:
        v.copy_(fill)
    return v, buf


def _guards_intact(buf, what, value=float("nan")):
    fresh = torch.full((GUARD,), value, dtype=buf.dtype, device=DEV)
    assert torch.equal(_bits(buf[:GUARD]), _bits(fresh)), f"{what}: wrote BEFORE the tensor"
    assert torch.equal(_bits(buf[-GUARD:]), _bits(fresh)), f"{what}: wrote PAST the tensor"


def _f32(v):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(DEV)


def _typed(v, t):
    """float64 numpy -> device tensor of type "bf16" / "f32" (the values are numbers of that type: assert_premises)"""
    return None if v is None else (X.to_bf16(v).to(DEV) if t == "bf16" else _f32(v))


class _Dev:
    """device operands of a case"""

    def __init__(self, c):
        d = X.operands(c)
        ti, tw, to = c.dt
        self.x, self.xbuf = _guarded(d["x"].shape, X.TORCH_DT[ti], _typed(d["x"], ti))
        self.w_clear = _f32(d["w"])
        self.images = {}
        self.bias, self.ab = _f32(d["bias"]), _f32(d["ab"])
        self.res, self.res_low = _typed(d.get("res"), to), _typed(d.get("res_low"), to)
        self.res_bias = _f32(d["coef"]) if "coef" in d else _f32(d.get("res_bias"))

    def image(self, c, w_paired):
        _, ops = _ops()
        if w_paired not in self.images:
            if w_paired == 2:
                self.images[2] = X.to_bf16(X.operands(c)["w"]).to(DEV).contiguous()
            elif w_paired == 1:
                self.images[1] = ops.pw_pack_weight_paired(self.w_clear)
            else:
                self.images[0] = ops.pw_pack_weight(self.w_clear, X.TORCH_DT[c.dt[1]])
        return self.images[w_paired]


def _mode_kw(c, dv):
    nat, _ = _ops()
    kw = dict(act=nat.ACT_GELU if c.act == "gelu" else nat.ACT_NONE, pre_act=nat.ACT_GELU if c.pre_gelu else nat.ACT_NONE)
    if c.gather:
        kw.update(gather=2, grid=c.gather)
    if c.res == "add":
        kw.update(res=dv.res, res_mode=nat.RES_ADD)
    elif c.res == "gelu_bwd":
        kw.update(res=dv.res, res_mode=nat.RES_GELU_BWD)
    elif c.res in ("norm_bwd", "norm_bwd_crop"):
        kw.update(res=dv.res, res_mode=nat.RES_NORM_BWD, res_bias=dv.res_bias)
        if c.res == "norm_bwd_crop":
            kw.update(grid=c.grid)
    elif c.res in ("up", "up_low"):
        kw.update(res=dv.res, res_mode=nat.RES_UPSAMPLE, grid=c.grid, res_low=dv.res_low, res_bias=dv.res_bias)
    return kw


def _launch(c, dv, w_paired):
    _, ops = _ops()
    y, ybuf = _guarded(c.out_shape, X.TORCH_DT[c.dt[2]])
    ops.pw_conv(dv.x, dv.image(c, w_paired), dv.bias, N=c.N, rows_per_sample=c.rows, c_in=c.cin, c_out=c.cout, out_dtype=y.dtype, ab=dv.ab,
                y=y, w_paired=w_paired, **_mode_kw(c, dv))
    torch.cuda.synchronize()
    _guards_intact(ybuf, c.id)
    return y


def _args(c, w_paired=None):
    """the shape / dtype / mode fields of pytc_pw_args for a case (no pointers: the *_supported entries do not inspect them)"""
    nat, _ = _ops()
    code = {"f32": nat.F32, "bf16": nat.BF16}
    a = nat.PwArgs()
    a.N, a.rows_per_sample, a.C_in, a.C_out = c.N, c.rows, c.cin, c.cout
    a.in_dtype, a.w_dtype, a.out_dtype = (code[t] for t in c.dt)
    a.act = nat.ACT_GELU if c.act == "gelu" else nat.ACT_NONE
    a.pre_act = nat.ACT_GELU if c.pre_gelu else nat.ACT_NONE
    a.gather = 2 if c.gather else 0
    a.res_mode = {"none": nat.RES_NONE, "add": nat.RES_ADD, "gelu_bwd": nat.RES_GELU_BWD, "norm_bwd": nat.RES_NORM_BWD,
                  "norm_bwd_crop": nat.RES_NORM_BWD, "up": nat.RES_UPSAMPLE, "up_low": nat.RES_UPSAMPLE}[c.res]
    a.Di, a.Hi, a.Wi = c.gather or c.grid or (0, 0, 0)
    a.w_paired = c.w_paired if w_paired is None else w_paired
    return a


def _alternatives(c):
    """the other weight images / knob settings under which the SAME operands must give the same bits: (w_paired, knobs, instance)"""
    out = []
    if X.expected_instance(c).startswith(("pw_stem", "pw_head")):
        out.append((0, dict(pw_thin=0)))
    if c.form in ("paired", "rowmajor"):
        if "norm_bwd" not in c.res:
            out.append((0, {}))                                     # the unpaired image on the generic kernel
        if c.form == "rowmajor" and X.paired_supported(c):
            out.append((1, {}))
    return out


def _run_case(c):
    nat, ops = _ops()
    ref = X.assert_premises(c)
    lib = nat.lib()
    assert bool(lib.pytc_pw_conv_paired_supported(ctypes.byref(_args(c)))) == X.paired_supported(c), f"{c.id}: paired_supported"
    assert bool(lib.pytc_pw_conv_rowmajor_supported(ctypes.byref(_args(c)))) == X.rowmajor_supported(c), f"{c.id}: rowmajor_supported"
    dv = _Dev(c)
    with _knobs(**X.KNOB_DEFAULTS):
        first = _launch(c, dv, c.w_paired)
        with ops.profiled() as prof:                      # the profiler's kernel family of the launch, as far as hip_ops tells them apart
            again = _launch(c, dv, c.w_paired)
        symbols = set(prof.by_symbol())
    assert symbols == ({"pw_gemm_lds_kernel"} if c.w_paired == 2 else {"pw_conv_fwd"}), f"{c.id}: profiler symbols {symbols}"
    assert not torch.isnan(first.float()).any(), f"{c.id}: {int(torch.isnan(first.float()).sum())} outputs were never written"
    X.check_bits(first, ref["y"], f"{c.id} [{X.expected_instance(c)}]")
    assert torch.equal(_bits(again), _bits(first)), f"{c.id}: does not repeat"
    for w_paired, knobs in _alternatives(c):
        with _knobs(**knobs):
            other = _launch(c, dv, w_paired)
        inst = X.expected_instance(c, thin=knobs.get("pw_thin", 1), w_paired=w_paired)
        assert inst != X.expected_instance(c)
        X.check_bits(other, ref["y"], f"{c.id} on the alternative [{inst}]")
    _guards_intact(dv.xbuf, c.id + " input")


@pytest.mark.parametrize("c", X.cases("generic"), ids=X.ids(X.cases("generic")))
def test_generic_mfma_kernel(c):
    _run_case(c)


@pytest.mark.parametrize("c", X.cases("stem"), ids=X.ids(X.cases("stem")))
def test_stem_kernel_and_its_fallback(c):
    _run_case(c)


@pytest.mark.parametrize("c", X.cases("head"), ids=X.ids(X.cases("head")))
def test_head_kernel_and_its_fallback(c):
    _run_case(c)


@pytest.mark.parametrize("c", X.cases("paired"), ids=X.ids(X.cases("paired")))
def test_paired_row_kernel(c):
    _run_case(c)


@pytest.mark.parametrize("c", X.cases("rowmajor"), ids=X.ids(X.cases("rowmajor")))
def test_rowmajor_lds_gemm(c):
    _run_case(c)


# ------------------------------------------------------------------------------------------------------------- packers
@pytest.mark.parametrize("transposed", [False, True], ids=["plain", "transposed"])
@pytest.mark.parametrize("tw", ["bf16", "f32"])
def test_pack_weight_image_whole(tw, transposed):
    nat, ops = _ops()
    rng = np.random.default_rng(5)
    for cout, cin in ((13, 20), (40, 48), (3, 1), (1, 64), (80, 13), (32, 32)):
        # distinct values that both types hold: k / 4 for k < 2^8 ... small integers otherwise
        w = (rng.permutation(cout * cin).astype(np.float64).reshape(cout, cin) % 251 - 125) / 4 + (1.0 + 2.0 ** -10 if tw == "f32" else 0.0)
        src = _f32(w.T if transposed else w)
        img = ops.pw_pack_weight(src, X.TORCH_DT[tw], transposed=transposed)
        code = nat.F32 if tw == "f32" else nat.BF16
        assert nat.lib().pytc_pw_packed_elems(cout, cin, code) == X.packed_elems_model(cout, cin, tw) == img.numel()
        want = X.packed_model(w, tw)
        X.check_bits(img, X.to_bf16(want) if tw == "bf16" else torch.from_numpy(want.astype(np.float32)), f"pack {tw} {cout}x{cin}")
        assert int((img == 0).sum()) >= img.numel() - cout * cin                       # the padding is zero
    assert nat.lib().pytc_pw_packed_elems(0, 4, nat.BF16) == -1 and nat.lib().pytc_pw_packed_elems(4, 4, 7) == -1


@pytest.mark.parametrize("transposed", [False, True], ids=["plain", "transposed"])
def test_pack_weight_paired_image_whole(transposed):
    _, ops = _ops()
    rng = np.random.default_rng(6)
    for cout, cin in ((32, 32), (96, 64), (64, 40), (256, 1024)):
        w = (rng.permutation(cout * cin).astype(np.float64).reshape(cout, cin) % 251 - 125) / 4
        img = ops.pw_pack_weight_paired(_f32(w.T if transposed else w), transposed=transposed)
        X.check_bits(img, X.to_bf16(X.packed_paired_model(w)), f"paired pack {cout}x{cin}")


# ------------------------------------------------------------------------------------------------------------- refusals
SENTINEL = 7.0


def _refused(c, what, *, w_paired=None, drop=(), **over):
    """the call must fail with a message and leave the sentinel-filled output untouched"""
    nat, ops = _ops()
    dv = _Dev(c)
    wp = c.w_paired if w_paired is None else w_paired
    odt = over.pop("out_dtype", X.TORCH_DT[c.dt[2]])
    y, ybuf = _guarded(c.out_shape, odt, value=SENTINEL)
    kw = dict(N=c.N, rows_per_sample=c.rows, c_in=c.cin, c_out=c.cout, out_dtype=odt, ab=dv.ab, y=y, w_paired=wp, **_mode_kw(c, dv))
    kw.update(over)
    for k in drop:
        kw[k] = None
    with pytest.raises(RuntimeError) as err:
        ops.pw_conv(dv.x, dv.image(c, wp), dv.bias, **kw)
    torch.cuda.synchronize()
    msg = str(err.value)
    assert "pw_conv" in msg and not msg.rstrip().endswith("?") and len(msg) > 30, f"{what}: no message ({msg!r})"
    assert torch.equal(_bits(ybuf), _bits(torch.full_like(ybuf, SENTINEL))), f"{what}: the refused call wrote its output"


def test_refusals_leave_the_output_untouched():
    nat, _ = _ops()
    B3, F3 = X.B3, X.GENERIC_ROUTES[0]
    C = X.Case
    plain = C("generic", "refusal", B3, 64, 128, 2, 48)
    _refused(C("generic", "r", B3, 96, 64, 2, 48), "w_paired = 1 with C_in = 96", w_paired=1)
    _refused(C("generic", "r", B3, 64, 64, 2, 48), "w_paired = 1 with an activation", w_paired=1, act=nat.ACT_SIGMOID)
    _refused(C("generic", "r", B3, 32, 128, 2, 48), "w_paired = 2 with C_in = 32", w_paired=2)
    _refused(C("generic", "r", B3, 64, 64, 2, 48), "w_paired = 2 with C_out = 64", w_paired=2)
    _refused(C("generic", "r", B3, 64, 128, 2, 12, gather=(3, 4, 5)), "w_paired = 2 with a gather", w_paired=2)
    _refused(plain, "w_paired = 2 with an activation", w_paired=2, act=nat.ACT_GELU)
    up = C("generic", "r", B3, 64, 128, 2, 48, res="up_low", grid=(2, 4, 6))
    for wp in (0, 1):
        _refused(up, "gather = 2 with RES_UPSAMPLE", w_paired=wp, gather=2)
        _refused(up, "RES_UPSAMPLE on an odd grid", w_paired=wp, grid=(2, 3, 8))
        _refused(up, "RES_UPSAMPLE on a grid that does not match the rows", w_paired=wp, grid=(2, 4, 8))
        _refused(C("generic", "r", B3, 64, 128, 2, 12, gather=(3, 4, 5)), "a gather grid that does not match the rows", w_paired=wp, grid=(3, 4, 7))
    nb = C("generic", "r", B3, 64, 128, 2, 60, bias=False, res="norm_bwd")
    _refused(nb, "RES_NORM_BWD without w_paired", w_paired=0)
    for wp in (1, 2):
        _refused(nb, "RES_NORM_BWD without res_bias", w_paired=wp, drop=("res_bias",))
        _refused(nb, "a crop grid that does not match the rows", w_paired=wp, grid=(3, 4, 6))
        _refused(nb, "a crop grid with a one-voxel axis", w_paired=wp, grid=(1, 6, 10))
    for wp in (0, 1, 2):
        _refused(C("generic", "r", B3, 64, 128, 2, 48, res="add"), "a residual mode without a residual pointer", w_paired=wp, drop=("res",))
        _refused(plain, "a bad pre_act", w_paired=wp, pre_act=nat.ACT_SIGMOID)
    _refused(C("generic", "r", F3, 20, 12, 2, 17), "f32 input, f32 weights, bf16 output", out_dtype=bf)
    # activation codes that apply_act does not evaluate (they used to pass through as the identity)
    for code in (nat.ACT_RELU, nat.ACT_LEAKY, nat.ACT_ELU, nat.ACT_SOFTMAX, 99):
        _refused(C("generic", "r", B3, 24, 13, 2, 17), f"act = {code}", act=code)
        _refused(C("generic", "r", B3, 1, 8, 2, 17), f"act = {code} on the stem kernel", act=code)

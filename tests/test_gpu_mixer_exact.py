"""The fused channel mixers against the bit model of the packed-fp16 GELU and fp64 references with NO tolerance
(tests/mixer_exact_cases.py): on the operands filed there every product and every partial sum of both GEMMs and of the epilogue is an
fp32 number in any order, the hidden activation is a fixed chain of IEEE fp16 operations, and the only rounding of an output is its
store -- so pw_mlp_kernel in its 13 instances (affine / folded operands, no residual / RES_ADD / RES_UPSAMPLE with and without res_low,
the HEAD, STEMRES and STOREH instances), pw_mlp_dma_kernel (plain, add, stem residual, head, projection; every mlp_dma_wgs), the
LDS-resident and chunk-streamed kernels, the pw_gemm pair and the fused block (dwmix) must give the reference's BITS: every output,
stored hidden pre-activation, f16 hidden and logit.

test_gelu_bits_* sweep the hidden activation itself: every finite f16 input in [-8, 8], larger ones up to saturation, fp32 inputs
either side of f16 rounding midpoints and inputs with subnormal f16 images, through pw_gemm(gelu=True) (which returns the f16 hidden)
and through the 32 -> 32 -> 32 mixer (two launches recover the eleven bits from bf16 outputs).

Each case asserts its premises (mixer_exact_cases.assert_premises, the helper the host proof uses), runs twice and must repeat bit for
bit; inputs, residuals and -- wherever the wrapper takes an output buffer -- outputs lie inside NaN-filled buffers with guard rows; with
N = 3 the last sample run alone must give the bits it has in the batch.  Knobs are set through ops.set_tuning inside try / finally.
What these cases cannot see is listed in DESIGN.md 4.2b; tests/test_host_mixer_exact_cases.py proves that sixteen seeded defects each
fail; profiles/mixer_exact_seeded_defects.txt records six defects put into the kernels themselves and the cases of this file that went
red.  pw_mlp_up is not here: its entry takes the bf16 projection image only, i.e. the exp + rcp GELU, which has no exact form.  The whole
file takes about 6 s on an MI355X, the slowest case 0.6 s."""
import contextlib
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import mixer_exact_cases as X  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096          # elements either side of every guarded tensor
bf = torch.bfloat16


def _ops():
    from pytorch_connectomics_amd import _native as nat, hip_ops as ops
    return nat, ops


def _ids(cs):
    return [c.id for c in cs]


@contextlib.contextmanager
def _knobs(knobs):
    _, ops = _ops()
    try:
        for k, v in knobs:
            ops.set_tuning(k, v)
        yield
    finally:
        for k, v in X.KNOB_DEFAULTS.items():
            ops.set_tuning(k, v)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _guarded(shape, dtype, fill=None):
    """(view of `shape`, whole buffer): the view sits GUARD elements inside a NaN-filled buffer"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    v = buf[GUARD:GUARD + n].view(tuple(shape))
    if fill is not None:
        v.copy_(fill)
    return v, buf


def _guards_intact(buf, what):
    fresh = torch.full((GUARD,), float("nan"), dtype=buf.dtype, device=DEV)
    assert torch.equal(_bits(buf[:GUARD]), _bits(fresh)), f"{what}: wrote BEFORE the tensor"
    assert torch.equal(_bits(buf[-GUARD:]), _bits(fresh)), f"{what}: wrote PAST the tensor"


_check = X.check_bits


def _f32(v):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(DEV)


class _Dev:
    """device operands of a case for samples [n0, n0 + N)"""

    def __init__(self, c, n0=0, N=None):
        _, ops = _ops()
        d = X.operands(c)
        N = c.N - n0 if N is None else N
        sl = slice(n0, n0 + N)
        self.N, self.bufs = N, []
        self.t = self._g(X.to_bf16(d["t"][sl]))
        self.folded = d["ab"] is None
        if self.folded:
            self.ab = None
            self.w2 = torch.stack([ops.pw_pack_weight_paired(_f32(d["w2"][n])) for n in range(n0, n0 + N)])
            self.b2 = _f32(d["b2"][sl])
        else:
            self.ab = _f32(d["ab"][sl])
            self.w2 = ops.pw_pack_weight_paired(_f32(d["w2"]))
            self.b2 = _f32(d["b2"])
        self.w3_clear = _f32(d["w3"])
        self.w3 = ops.pw_pack_weight_paired(self.w3_clear, f16=True)
        self.b3 = _f32(d["b3"])
        self.res = self._g(X.to_bf16(d["res"][sl])) if "res" in d else None
        self.res_low = self._g(X.to_bf16(d["res_low"][sl])) if "res_low" in d else None
        self.res_bias = _f32(d.get("res_bias"))
        if c.res == "stem":
            self.x0, self.stem_w, self.stem_b = self._g(_f32(d["x0"][sl])), _f32(d["stem_w"]), _f32(d["stem_b"])
        if c.n_head:
            self.head_w, self.head_b = ops.pack_head_fragment(_f32(d["head_w"])), _f32(d["head_b"])
        if c.proj:
            self.proj_w, self.proj_b = ops.pw_pack_weight_paired(_f32(d["proj_w"])), _f32(d["proj_b"])

    def _g(self, fill):
        v, buf = _guarded(fill.shape, fill.dtype, fill)
        self.bufs.append(buf)
        return v


def _res_kw(c, dv):
    nat, _ = _ops()
    if c.res == "add":
        return dict(res=dv.res, res_mode=nat.RES_ADD)
    if c.res in ("up", "up_low"):
        return dict(res=dv.res, res_mode=nat.RES_UPSAMPLE, grid=c.grid, res_low=dv.res_low, res_bias=dv.res_bias)
    return {}


def _launch(c, dv, **extra):
    """the case's entry point -> dict of outputs (y may be None); y lies in a guarded buffer where the wrapper takes one"""
    nat, ops = _ops()
    kw = dict(N=dv.N, rows_per_sample=c.rows, c_in=c.cin, c_hid=c.chid, c_out=c.cout)
    out = {}
    if c.n_head:
        for store_y in (False, True):
            y, lg = ops.pw_mlp_head(dv.t, dv.ab, dv.w2, dv.b2, dv.w3, dv.b3, dv.head_w, dv.head_b, res=dv.res, store_y=store_y, **kw)
            assert (y is None) == (not store_y)
            out["logits" if store_y else "logits_nostore"] = lg
            if store_y:
                out["y"] = y
        return out
    if c.proj:
        for store_y in (False, True):
            y, z = ops.pw_mlp_proj(dv.t, dv.w2, dv.b2, dv.w3, dv.b3, dv.proj_w, dv.proj_b, res=dv.res, store_y=store_y, **kw)
            assert (y is None) == (not store_y)
            out["z" if store_y else "z_nostore"] = z
            if store_y:
                out["y"] = y
        return out
    y, ybuf = _guarded((dv.N, c.rows, c.cout), bf)
    if c.res == "stem":
        ops.pw_mlp_stemres(dv.t, dv.ab, dv.w2, dv.b2, dv.w3, dv.b3, dv.x0, dv.stem_w, dv.stem_b, y=y, **kw)
    else:
        ops.pw_mlp(dv.t, dv.ab, dv.w2, dv.b2, dv.w3, dv.b3, y=y, **_res_kw(c, dv), **kw, **extra)
    torch.cuda.synchronize()
    _guards_intact(ybuf, c.id)
    out["y"] = y
    return out


def _want(c, ref, key):
    if key.startswith("logits"):
        return ref["logits"]
    if key.startswith("z"):
        return ref["z"]
    return ref[key]


def _run_case(c, **extra):
    ref = X.assert_premises(c)
    with _knobs(c.knobs):
        dv = _Dev(c)
        first = _launch(c, dv, **extra)
        again = _launch(c, dv, **extra)
        for k, v in first.items():
            _check(v, _want(c, ref, k), f"{c.id}: {k}")
            assert torch.equal(_bits(again[k]), _bits(v)), f"{c.id}: {k} does not repeat"
        if c.N == 3:                     # the last sample alone: the bits it has in the batch
            d1 = _Dev(c, n0=2, N=1)
            for k, v in _launch(c, d1, **extra).items():
                _check(v, _want(c, ref, k)[2:3], f"{c.id}: {k} of the last sample run alone")
    return ref


# ------------------------------------------------------------------------------------------------------------- the GELU sweep
def _sweep():
    groups = X.sweep_inputs()
    x = np.concatenate(list(groups.values()))
    return x, X.gelu_h8_model(x)


def _report(x, got16, want16, what):
    bad = got16.view(np.uint16) != want16.view(np.uint16)
    if not bad.any():
        return
    i = np.nonzero(bad)[0]
    first = [f"x = {float(x[j])!r}: kernel {float(got16[j])!r} model {float(want16[j])!r}" for j in i[:8]]
    raise AssertionError(f"{what}: {len(i)} of {len(x)} hidden activations differ from the bit model; " + "; ".join(first))


def test_gelu_bits_through_the_gemm_epilogue():
    """pw_gemm(gelu=True) returns the f16 hidden itself.  x = hi + mid + lo (three bf16 pieces, exact for any fp32 x) through a
    [I | I | I] weight: the pieces sit in different 64-wide k steps, so the fp32 accumulator is 0 + hi + mid + lo in k order -- exact."""
    _, ops = _ops()
    x, want = _sweep()
    n = len(x)
    rows = (n + 63) // 64
    xp = np.zeros(rows * 64, np.float32)
    xp[:n] = x
    x64 = xp.astype(np.float64)
    hi = X.bf16_np(_as_f32(x64))
    mid = X.bf16_np(_as_f32(x64 - hi))
    lo = x64 - hi - mid
    assert (X.bf16_np(lo) == lo).all()
    s = (np.float32(0) + hi.astype(np.float32)) + mid.astype(np.float32)
    assert ((s + lo.astype(np.float32)) == xp).all()                         # the premise: the accumulator holds x exactly
    t = np.concatenate([hi.reshape(rows, 64), mid.reshape(rows, 64), lo.reshape(rows, 64)], 1)
    w = np.zeros((128, 192))
    for o in range(128):
        w[o, [o % 64, 64 + o % 64, 128 + o % 64]] = 1.0
    tv, tbuf = _guarded((1, rows, 192), bf, X.to_bf16(t)[None])
    zero = torch.zeros(128, device=DEV)
    for rk in (0, 64, 128):
        with _knobs((("pw_gemm_rows", rk),)):
            h = ops.pw_gemm(tv, X.to_bf16(w).to(DEV), zero, N=1, rows_per_sample=rows, gelu=True)
        assert h.dtype == torch.float16
        got = h.cpu().numpy().reshape(rows, 128)
        _report(x, got[:, :64].reshape(-1)[:n], want, f"pw_gemm_rows = {rk}")
        assert (got[:, :64].view(np.uint16) == got[:, 64:].view(np.uint16)).all()


def _as_f32(v):
    """the fp32 image of a float64 value as float64 (exact here: an fp32 number, or such a number less its leading bf16 piece)"""
    return v.astype(np.float32).astype(np.float64)


def test_gelu_bits_through_the_fused_mixer():
    """pw_mlp 32 -> 32 -> 32 with per-sample operands: W2_n = 0 and b2_n = x put ANY fp32 x into the accumulator; W3 = I.  The bf16
    output hides three of the hidden's eleven bits: a second launch with the residual -y1 gives bf16(g - y1) = g - y1 exactly, so
    g = y1 + y2.  (The sum cannot tell -0 from +0: VALUES are compared here; the route through pw_gemm compares the bit patterns.)"""
    nat, ops = _ops()
    x, want = _sweep()
    n = len(x)
    N = (n + 31) // 32
    xp = np.zeros(N * 32, np.float32)
    xp[:n] = x
    t = torch.zeros((N, 1, 32), dtype=bf, device=DEV)
    w2n = torch.zeros((N, 32 * 32), dtype=bf, device=DEV)
    b2n = torch.from_numpy(xp.reshape(N, 32)).to(DEV)
    w3 = ops.pw_pack_weight_paired(torch.eye(32, device=DEV), f16=True)
    zero = torch.zeros(32, device=DEV)
    kw = dict(N=N, rows_per_sample=1, c_in=32, c_hid=32, c_out=32)
    y1 = ops.pw_mlp(t, None, w2n, b2n, w3, zero, **kw)
    y2 = ops.pw_mlp(t, None, w2n, b2n, w3, zero, res=-y1, res_mode=nat.RES_ADD, **kw)
    y1f, y2f = y1.float().cpu().numpy().reshape(-1)[:n], y2.float().cpu().numpy().reshape(-1)[:n]
    w32 = want.astype(np.float32)
    # the recovery is exact whenever the kernel is right: bf16(g) is within eight bits of g, the remainder has at most four
    assert (X.bf16_np((w32 - X.bf16_np(w32)).astype(np.float64)) == (w32 - X.bf16_np(w32))).all()
    got = y1f + y2f
    bad = got != w32
    if bad.any():
        i = np.nonzero(bad)[0]
        first = [f"x = {float(x[j])!r}: kernel {float(got[j])!r} (y1 {float(y1f[j])!r}) model {float(w32[j])!r}" for j in i[:8]]
        raise AssertionError(f"{len(i)} of {n} hidden activations differ from the bit model; " + "; ".join(first))


# ------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("c", X.cases("stream"), ids=_ids(X.cases("stream")))
def test_streaming_mixer(c):
    _run_case(c)


@pytest.mark.parametrize("c", X.cases("dma"), ids=_ids(X.cases("dma")))
def test_dma_mixer_and_epilogue_forms(c):
    _run_case(c)


@pytest.mark.parametrize("c", X.cases("lds"), ids=_ids(X.cases("lds")))
def test_lds_resident_mixer(c):
    _, ops = _ops()
    assert ops.pw_mlp_lds_supported(c.cin, c.chid, c.cout)
    _run_case(c, lds=True)


@pytest.mark.parametrize("c", X.cases("chunk"), ids=_ids(X.cases("chunk")))
def test_chunk_streamed_mixer(c):
    _, ops = _ops()
    assert ops.pw_mlp_chunk_supported(c.cin, c.chid, c.cout)
    _run_case(c, chunked=True)


@pytest.mark.parametrize("c", X.cases("gemm"), ids=_ids(X.cases("gemm")))
def test_gemm_pair(c):
    """the f16 hidden whole against the model, then the projection with its residual mode"""
    _, ops = _ops()
    ref = X.assert_premises(c)
    d = X.operands(c)
    dv = _Dev(c)
    kw = dict(N=c.N, rows_per_sample=c.rows)
    want_h = torch.from_numpy(ref["g"].copy())
    with _knobs(c.knobs):
        outs = []
        for _ in range(2):
            h, hbuf = _guarded((c.N, c.rows, c.chid), torch.float16)
            y, ybuf = _guarded((c.N, c.rows, c.cout), bf)
            ops.pw_gemm(dv.t, X.to_bf16(d["w2"]).to(DEV), dv.b2, ab=dv.ab, gelu=True, y=h, **kw)
            ops.pw_gemm(h, dv.w3_clear.to(torch.float16).contiguous(), dv.b3, y=y, **_res_kw(c, dv), **kw)
            torch.cuda.synchronize()
            _guards_intact(hbuf, c.id + " hidden")
            _guards_intact(ybuf, c.id)
            outs.append((h, y))
    _check(outs[0][0], want_h, f"{c.id}: f16 hidden")
    _check(outs[0][1], ref["y"], f"{c.id}: y")
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1])), f"{c.id}: does not repeat"


@pytest.mark.parametrize("c", X.cases("conv"), ids=_ids(X.cases("conv")))
def test_conversion_into_the_hidden(c):
    """h is neither an f16 nor a bf16 number: the inference kernels convert it toward zero; the training forward stores bf16(h),
    evaluates GELU AT THE STORED VALUE, and its store-free form gives the same y"""
    _, ops = _ops()
    _run_case(c)
    if c.form == "folded":
        return                                  # the training kernels take the shared expand image and the affine
    ref = X.assert_premises(c, True)
    assert not torch.equal(ref["y"], X.reference(c)["y"])
    dv = _Dev(c)
    kw = dict(N=c.N, rows_per_sample=c.rows, c_in=c.cin, c_hid=c.chid, c_out=c.cout)
    for _ in range(2):
        hp, hbuf = _guarded((c.N, c.rows, c.chid), bf)
        y, ybuf = _guarded((c.N, c.rows, c.cout), bf)
        y2, y2buf = _guarded((c.N, c.rows, c.cout), bf)
        ops.pw_mlp(dv.t, dv.ab, dv.w2, dv.b2, dv.w3, dv.b3, y=y, hidden_pre=hp, **_res_kw(c, dv), **kw)
        ops.pw_mlp(dv.t, dv.ab, dv.w2, dv.b2, dv.w3, dv.b3, y=y2, train_nostore=True, **_res_kw(c, dv), **kw)
        torch.cuda.synchronize()
        for b in (hbuf, ybuf, y2buf):
            _guards_intact(b, c.id + " training forward")
        _check(hp, ref["hidden_pre"], f"{c.id}: stored hidden pre-activation")
        _check(y, ref["y"], f"{c.id}: training forward y")
        _check(y2, ref["y"], f"{c.id}: store-free training forward y")


def _fused_block(c, n0=0):
    """ops.dwmix on samples [n0, N) of the case -> dict of outputs; x and y inside NaN-filled buffers"""
    _, ops = _ops()
    d = X.operands(c)
    N = c.N - n0
    shape = (N,) + tuple(c.dims)
    x, xbuf = _guarded(shape + (32,), bf, X.to_bf16(d["x5"][n0:]))
    assert ops.dwmix_supported(x, c.chid, 32)
    w2n = torch.stack([ops.pw_pack_weight_paired(_f32(d["w2"][n])) for n in range(n0, c.N)])
    w3 = ops.pw_pack_weight_paired(_f32(d["w3"]), f16=True)
    args = (x, _f32(d["taps"]), _f32(d["dw_bias"]), w2n, _f32(d["b2"][n0:]), w3, _f32(d["b3"]))
    out = {}
    if c.n_head:
        hw, hb = ops.pack_head_fragment(_f32(d["head_w"])), _f32(d["head_b"])
        for store_y in (False, True):
            y, ybuf = _guarded(shape + (32,), bf)
            got, lg = ops.dwmix(*args, c_hid=c.chid, residual=c.res == "add", y=y if store_y else None, head_w=hw, head_b=hb, store_y=store_y)
            torch.cuda.synchronize()
            _guards_intact(ybuf, c.id)
            assert (got is None) == (not store_y)
            out["logits" if store_y else "logits_nostore"] = lg.view(N, c.rows, c.n_head)
            if store_y:
                out["y"] = y.view(N, c.rows, 32)
        return out
    y, ybuf = _guarded(shape + (32,), bf)
    ops.dwmix(*args, c_hid=c.chid, residual=c.res == "add", y=y)
    torch.cuda.synchronize()
    _guards_intact(ybuf, c.id)
    return {"y": y.view(N, c.rows, 32)}


@pytest.mark.parametrize("c", X.cases("dwmix"), ids=_ids(X.cases("dwmix")))
def test_fused_block(c):
    """dwmix: isolated +-1 voxels and +-1 taps keep the depthwise result in {0, +-1} + a half, the mixer's operands are the filed ones
    (mixer_exact_cases._dwmix_cases): block output and logits carry the reference's bits"""
    ref = X.assert_premises(c)
    with _knobs(c.knobs):
        first, again = _fused_block(c), _fused_block(c)
        for k, v in first.items():
            _check(v, _want(c, ref, k), f"{c.id}: {k}")
            assert torch.equal(_bits(again[k]), _bits(v)), f"{c.id}: {k} does not repeat"
        if c.N == 3:
            for k, v in _fused_block(c, n0=2).items():
                _check(v, _want(c, ref, k)[2:3], f"{c.id}: {k} of the last sample run alone")

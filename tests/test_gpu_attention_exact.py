"""The ViT and Swin attention kernels and the LDS-tiled linear GEMM (csrc/transformer_kernels.hip) against references with NO tolerance
(tests/attention_exact_cases.py): code-word queries and keys make every softmax probability exactly 1 or exactly 0 in fp32, so the
forward's O must reproduce fl32(fl32(sum of the members' V) * fl32(1 / |M|)), rounded once to the storage type, bit for bit over
the whole tensor, at N below, at and above every multiple of the 64-key tile, in every (dtype, D, WIN) instantiation.

  one-hot sets (selector, selector_neg, rescale_up / rescale_down, Swin selector): O, lse (= the scaled score; Swin at d = 32 to 2
      fp32 ulps, where the scaled score is not representable and contracting the scale multiply with the bias add is the compiler's
      choice), dvec and the whole dqkv (dV integer sums, dQ = dK = 0), and for Swin dtable = 0, all with torch.equal.
  group sets: O with torch.equal; lse against m + log |M| in fp64 to 4 fp32 ulps; dQ / dK / dV / dtable per element against the fp64
      closed form within attention_exact_cases.grad_tolerance -- a bound derived from the arithmetic, dominated by the half ulp of
      the saved lse (magnitude up to 1536) that the recomputed P = expf(sc - lse) inherits; table rows no pair reads exactly 0.
      The Swin member sets are cut by the bias table (0 / -256) and by the shift-region labels, so O reads
      relative_position_index[:n, :n] and compute_mask's labels exactly.  A key excluded by the mask alone keeps expf(-100), a
      denormal of about 3.7e-44 or 0: absorbed exactly, since V >= 1 and every row sum is at least 1.

Every output (out, lse, dvec, dqkv, partial, dtable; y, dx, dw, db, dpos) is a view inside a larger NaN-filled buffer, as in
tests/test_gpu_dense_conv_exact.py: an element no thread writes stays NaN, a write past either end changes a guard word; every
operand (qkv, dout, the bias table; x, w, dy, ...) sits inside a NaN-filled buffer too, so a read past a tensor's end that reaches
an accumulator poisons it.  Each case runs twice and must repeat bit for bit.  One more test per path sends the selector inputs
through AttentionFn / WindowAttentionFn and holds the wrappers to the same exact result.

What these cases cannot see: dQ / dK / dV / dtable VALUES at the group sets are bounded, not exact; the GELU flags of the GEMM
and LayerNorm have no exact form (rsqrtf, erff) and stay with the tolerance tests of test_gpu_unetr.py / test_gpu_swin_unetr.py."""
import ctypes as C
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import attention_exact_cases as X  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096          # elements either side of an output tensor
IN_GUARD = 8192       # elements either side of an operand


def _nat():
    from pytorch_connectomics_amd import _native as nat
    return nat


def _ids(cs):
    return [c.id for c in cs]


def _numel(shape):
    n = 1
    for v in shape:
        n *= int(v)
    return n


def _out(shape, dtype):
    """-> (view of `shape` inside a NaN-filled buffer, the buffer)"""
    n = _numel(shape)
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    return buf[GUARD:GUARD + n].view(shape), buf


def _inp(t: torch.Tensor, dtype):
    """the operand in `dtype` on the device, NaN on both sides of it"""
    n = t.numel()
    buf = torch.full((n + 2 * IN_GUARD,), float("nan"), dtype=dtype, device=DEV)
    v = buf[IN_GUARD:IN_GUARD + n].view(t.shape)
    v.copy_(t.to(dtype))
    return v


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _guards_ok(buf: torch.Tensor, what: str) -> None:
    fresh = torch.full((GUARD,), float("nan"), dtype=buf.dtype, device=DEV)
    assert torch.equal(_bits(buf[:GUARD]), _bits(fresh)), f"{what}: wrote BEFORE the tensor"
    assert torch.equal(_bits(buf[-GUARD:]), _bits(fresh)), f"{what}: wrote PAST the tensor"
    assert not bool(buf[GUARD:-GUARD].isnan().any()), f"{what}: {int(buf[GUARD:-GUARD].isnan().sum())} elements have no writer (or are NaN)"


def _check(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    """torch.equal over the whole tensor; on failure the count and the first differing elements"""
    got = got.detach().cpu()
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), f"{what}: {got.dtype} {tuple(got.shape)}"
    if torch.equal(got, want):
        return
    bad = (got != want) | got.isnan()
    idx = bad.nonzero()
    first = [(tuple(i.tolist()), float(got[tuple(i)]), float(want[tuple(i)])) for i in idx[:8]]
    raise AssertionError(f"{what}: {len(idx)} of {got.numel()} elements differ (exact inputs: none may); first index, got, want: {first}")


def _within(got: torch.Tensor, ref: torch.Tensor, tol: torch.Tensor, what: str) -> None:
    err = (got.detach().cpu().double() - ref).abs()
    bad = ~(err <= tol)
    worst = float((err / tol.clamp_min(1e-300)).max())
    print(f"{what}: max |err| / bound = {worst:.3g}")
    if bool(bad.any()):
        idx = bad.nonzero()
        first = [(tuple(i.tolist()), float(got.detach().cpu().double()[tuple(i)]), float(ref[tuple(i)]), float(tol[tuple(i)])) for i in idx[:8]]
        raise AssertionError(f"{what}: {len(idx)} of {ref.numel()} elements outside the derived bound (worst {worst:.3g} x); "
                             f"first index, got, want, bound: {first}")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _code(dtype):
    nat = _nat()
    return nat.BF16 if dtype == X.BF16 else nat.F32


# ------------------------------------------------------------------------------------------------------------ the ABI calls
def _attention(c, dd):
    """pytc_attention_* / pytc_window_attention_* as ops.attention_fwd / bwd and ops.window_attention_fwd / bwd call them
    -> {name: view}, {name: buffer}"""
    nat = _nat()
    lib = nat.lib()
    qkv, dout = _inp(dd["qkv"], c.dtype), _inp(dd["dout"], c.dtype)
    rows = c.B * c.N
    v, b = {}, {}
    for name, shape, dt in (("out", (rows, c.hid), c.dtype), ("lse", (c.B, c.heads, c.N), X.F32), ("dvec", (c.B, c.heads, c.N), X.F32),
                            ("dqkv", (rows, 3 * c.hid), c.dtype)):
        v[name], b[name] = _out(shape, dt)
    p = lambda t: t.data_ptr()        # noqa: E731
    if c.win:
        table = _inp(dd["table"], X.F32)
        geom = (C.c_int32 * 12)(*c.geom)
        G = int(lib.pytc_window_attention_bias_groups(c.B, c.N, c.heads))
        assert 1 <= G <= c.B
        v["partial"], b["partial"] = _out((G, c.heads, c.N, c.N), X.F32)
        v["dtable"], b["dtable"] = _out((2197, c.heads), X.F32)
        nat.check(lib.pytc_window_attention_fwd(p(qkv), p(table), geom, p(v["out"]), p(v["lse"]), c.B, c.N, c.heads, c.d, c.scale,
                                                _code(c.dtype), _stream()), "window_attention_fwd")
        nat.check(lib.pytc_window_attention_bwd(p(qkv), p(table), geom, p(v["out"]), p(dout), p(v["lse"]), p(v["dvec"]), p(v["dqkv"]),
                                                p(v["partial"]), p(v["dtable"]), c.B, c.N, c.heads, c.d, c.scale, _code(c.dtype),
                                                _stream()), "window_attention_bwd")
    else:
        nat.check(lib.pytc_attention_fwd(p(qkv), p(v["out"]), p(v["lse"]), c.B, c.N, c.heads, c.d, c.scale, _code(c.dtype), _stream()),
                  "attention_fwd")
        nat.check(lib.pytc_attention_bwd(p(qkv), p(v["out"]), p(dout), p(v["lse"]), p(v["dvec"]), p(v["dqkv"]), c.B, c.N, c.heads, c.d,
                                         c.scale, _code(c.dtype), _stream()), "attention_bwd")
    torch.cuda.synchronize()
    return v, b


def _ulps(got: torch.Tensor, ref64: torch.Tensor) -> float:
    return float(((got.cpu().double() - ref64).abs() / X.ulp32(ref64)).max())


def _attention_exact(c, kind):
    what = f"{c.id} {kind}"
    dd = X.data(c, kind)
    o_want, m, lse64, cnt = X.forward_expected(c, dd)
    v, b = _attention(c, dd)
    for name, buf in b.items():
        _guards_ok(buf, f"{what} {name}")
    _check(v["out"], o_want, f"{what} O")
    # exact backward: every row one-hot -- but not a shifted Swin group set that happens to be, whose keys excluded by the mask alone
    # keep a denormal P in the backward (they go to the bounded branch, floor 1e-30)
    one_hot = int(cnt.max()) == 1 and not (c.win and kind.startswith("group") and any(c.shift))
    hid = c.hid
    if one_hot:
        if c.win and c.d == 32:
            u = _ulps(v["lse"], m.double())
            print(f"{what}: lse off by {u:.3g} fp32 ulps")
            assert u <= 2.0, f"{what} lse: {u} ulps from the scaled score"
        else:
            _check(v["lse"], m, f"{what} lse")
        ref = X.backward_reference(c, dd)
        assert float(ref["dqkv"][:, :2 * hid].abs().max()) == 0
        _check(v["dvec"], ref["dvec"].float(), f"{what} dvec")
        _check(v["dqkv"][:, 2 * hid:], ref["dqkv"][:, 2 * hid:].to(c.dtype), f"{what} dV")
        _check(v["dqkv"][:, :hid], torch.zeros(c.B * c.N, hid, dtype=c.dtype), f"{what} dQ")
        _check(v["dqkv"][:, hid:2 * hid], torch.zeros(c.B * c.N, hid, dtype=c.dtype), f"{what} dK")
        if c.win:
            _check(v["dtable"], torch.zeros(2197, c.heads), f"{what} dtable")
    else:
        u = _ulps(v["lse"], lse64)
        print(f"{what}: lse off by {u:.3g} fp32 ulps")
        assert u <= 4.0, f"{what} lse: {u} ulps from m + log |M|"
        ref = X.backward_reference(c, dd, o_store=o_want)
        d_tol = (c.d + 2) * X.EPS32 * ref["dvec"].abs()
        _within(v["dvec"], ref["dvec"], d_tol, f"{what} dvec")
        tol = X.grad_tolerance(c, ref["dqkv"], ref["abs"], ref["terms"], lse64, stored=True)
        for part, sl in (("dQ", slice(0, hid)), ("dK", slice(hid, 2 * hid)), ("dV", slice(2 * hid, 3 * hid))):
            _within(v["dqkv"][:, sl], ref["dqkv"][:, sl], tol[:, sl], f"{what} {part}")
        if c.win:
            _within(v["dtable"], ref["dtable"], X.grad_tolerance(c, ref["dtable"], ref["dtable_abs"], ref["dtable_terms"], lse64, stored=False),
                    f"{what} dtable")
    if c.win:
        used = torch.zeros(2197, dtype=torch.bool)
        used[X._rel(c.N).reshape(-1)] = True
        rest = v["dtable"].cpu()[~used]
        assert torch.equal(rest, torch.zeros_like(rest)), f"{what}: table rows no pair reads have a gradient"
    v2, _ = _attention(c, dd)
    for name in v:
        assert torch.equal(_bits(v2[name]), _bits(v[name])), f"{what} {name}: a second run differs from the first"


@pytest.mark.parametrize("c", X.vit_cases(), ids=_ids(X.vit_cases()))
def test_vit_attention_exact(c):
    for kind in c.sets:
        _attention_exact(c, kind)


@pytest.mark.parametrize("c", X.win_cases(), ids=_ids(X.win_cases()))
def test_window_attention_exact(c):
    for kind in c.sets:
        _attention_exact(c, kind)


# ------------------------------------------------------------------------------------------------- the autograd wrappers
@pytest.mark.parametrize("c", X.vit_cases(), ids=_ids(X.vit_cases()))
def test_vit_attention_wrapper_exact(c):
    from pytorch_connectomics_amd.training.transformer_autograd import AttentionFn
    dd = X.data(c, "selector")
    o_want, _, _, _ = X.forward_expected(c, dd)
    ref = X.backward_reference(c, dd)
    qkv = dd["qkv"].to(c.dtype).to(DEV).requires_grad_(True)
    o = AttentionFn.apply(qkv, c.B, c.heads)
    o.backward(dd["dout"].to(c.dtype).to(DEV))
    torch.cuda.synchronize()
    _check(o, o_want, f"{c.id} AttentionFn O")
    _check(qkv.grad, ref["dqkv"].to(c.dtype), f"{c.id} AttentionFn dqkv")


@pytest.mark.parametrize("c", X.win_cases(), ids=_ids(X.win_cases()))
def test_window_attention_wrapper_exact(c):
    from pytorch_connectomics_amd import hip_ops as ops
    from pytorch_connectomics_amd.training.swin_autograd import WindowAttentionFn
    assert ops.window_attention_geom(c.padded, c.ws, c.shift) == c.geom
    dd = X.data(c, "selector")
    o_want, _, _, _ = X.forward_expected(c, dd)
    ref = X.backward_reference(c, dd)
    qkv = dd["qkv"].to(c.dtype).to(DEV).requires_grad_(True)
    table = dd["table"].float().to(DEV).requires_grad_(True)
    o = WindowAttentionFn.apply(qkv, table, c.B, c.heads, c.geom)
    o.backward(dd["dout"].to(c.dtype).to(DEV))
    torch.cuda.synchronize()
    _check(o, o_want, f"{c.id} WindowAttentionFn O")
    _check(qkv.grad, ref["dqkv"].to(c.dtype), f"{c.id} WindowAttentionFn dqkv")
    _check(table.grad, torch.zeros(2197, c.heads), f"{c.id} WindowAttentionFn dtable")


# ------------------------------------------------------------------------------------------------------ the linear GEMM
def _gemm(c, dd):
    nat = _nat()
    lib = nat.lib()
    x, res, dy = (_inp(dd[k], c.dtype) for k in ("x", "res", "dy"))
    w, bias = _inp(dd["w"], X.F32), _inp(dd["bias"], X.F32)
    pos = _inp(dd["pos"], X.F32) if c.P else None
    v, b = {}, {}
    for name, shape, dt in (("y", (c.M, c.N), c.dtype), ("dx", (c.M, c.K), c.dtype), ("dw", (c.N, c.K), X.F32), ("db", (c.N,), X.F32)) + \
            ((("dpos", (c.P, c.N), X.F32),) if c.P else ()):
        v[name], b[name] = _out(shape, dt)
    p = lambda t: None if t is None else t.data_ptr()        # noqa: E731
    code = _code(c.dtype)
    nat.check(lib.pytc_linear_fwd(p(x), p(w), p(bias), p(pos), c.P, p(res), p(v["y"]), c.M, c.N, c.K, 0, code, _stream()), "linear_fwd")
    nat.check(lib.pytc_linear_bwd_data(p(dy), p(w), None, p(v["dx"]), c.M, c.N, c.K, code, _stream()), "linear_bwd_data")
    nat.check(lib.pytc_linear_wgrad(p(dy), p(x), p(v["dw"]), p(v["db"]), p(v.get("dpos")), c.P, c.M, c.N, c.K, 0, code, _stream()),
              "linear_wgrad")
    torch.cuda.synchronize()
    return v, b


@pytest.mark.parametrize("c", X.gemm_cases(), ids=_ids(X.gemm_cases()))
def test_linear_gemm_integer_exact(c):
    from pytorch_connectomics_amd import hip_ops as ops
    if c.dtype == X.BF16:              # these widths stay on pytc_linear_* in bf16 too: none takes the MFMA GEMM
        probe = torch.empty(0, dtype=X.BF16)
        assert not ops.linear_mfma_applies(probe, c.K, c.N) and not ops.linear_mfma_applies(probe, c.N, c.K)
    dd = X.gemm_data(c)
    ref = X.gemm_reference(c, dd)
    v, b = _gemm(c, dd)
    for name, buf in b.items():
        _guards_ok(buf, f"{c.id} {name}")
    for name in v:
        _check(v[name], ref[name].float().to(v[name].dtype), f"{c.id} {name}")
    v2, _ = _gemm(c, dd)
    for name in v:
        assert torch.equal(_bits(v2[name]), _bits(v[name])), f"{c.id} {name}: a second run differs from the first"

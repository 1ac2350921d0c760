"""Every GELU, sigmoid and tanh evaluation of the library over ALL 65 536 bf16 inputs (and, on fp32 routes, the 2^19-point fp32 grid)
against the interval models of tests/activation_domain_cases.py.  One test per row of its entry-point table: the operands around the
activation make everything else exact (host proof: tests/test_host_activation_domain_cases.py), so every stored output must lie inside
the model's [lo, hi] for its input, obey the class rules (finite in -> finite out, NaN in -> NaN out, the formulas' own values at
+-inf, +-0 -> +-0 and g'(+-0) = 1/2 exactly) and repeat bit for bit on a second launch.  Then the entry points the table files under the
same function, input type and rounding must agree BIT FOR BIT with each other on every finite input, no tolerance.

pw_conv and pw_mlp write into NaN-prefilled buffers with guard bands (they take their output tensors); gelu, grn_bwd_apply, linear_*,
pw_wgrad*, mixer_bwd_rc and pw_mlp_bwd allocate their own results inside hip_ops, so those launches have no guard bands (DESIGN.md 4.3c
lists this as a deviation; their out-of-bounds behaviour is the subject of the exact suites of their own families).
A failure names the entry point, the input bits and got / lo / hi.  PYTC_ACT_DOMAIN_REPORT=<file> appends the worst observed position
inside [lo, hi] per entry point (profiles/activation_domain_probe.txt keeps one such report, as information).  The whole file takes a
few seconds on an MI355X."""
import contextlib
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import activation_domain_cases as X  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096
TORCH_DT = {"bf16": torch.bfloat16, "f32": torch.float32}
KNOB_DEFAULTS = {"wgrad_valu": 0, "pw_thin": 1, "wgrad_dgrad_fused": 1}
_RESULTS = {}          # (entry id, sweep) -> (fp32 results shaped like the sweep, finite-input mask): shared by the bit-identity tests


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
        for k, v in KNOB_DEFAULTS.items():
            ops.set_tuning(k, v)


def _dev(v: np.ndarray, dt: str) -> torch.Tensor:
    """fp32 numpy values (numbers of type dt, or NaNs) -> device tensor of that type, bits kept"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    return (X.to_bf16_tensor(v) if dt == "bf16" else torch.from_numpy(v.copy())).to(DEV)


def _host(t: torch.Tensor) -> np.ndarray:
    torch.cuda.synchronize()
    return X.from_bf16_tensor(t) if t.dtype == torch.bfloat16 else t.detach().cpu().numpy().astype(np.float32, copy=True)


def _const(shape, value, dt):
    return torch.full(tuple(shape), value, dtype=TORCH_DT[dt], device=DEV)


def _f32(w: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(DEV)


def _guarded(shape, dtype):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    return buf[GUARD:GUARD + n].view(tuple(shape)), buf


def _guards_intact(buf, what):
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:GUARD].float()).all()), f"{what}: wrote BEFORE the tensor"
    assert bool(torch.isnan(buf[-GUARD:].float()).all()), f"{what}: wrote PAST the tensor"


def _pw_conv(e, x, w, *, c_in, c_out, w_paired=0, **kw):
    """ops.pw_conv on (R, c_in) rows with the fp64 weight matrix w (c_out, c_in), into a guarded NaN-prefilled output"""
    nat, ops = _ops()
    wdt = TORCH_DT["bf16" if (e.din == "bf16" or w_paired) else "f32"]
    if w_paired == 2:
        image = _f32(w).to(torch.bfloat16).contiguous()
    elif w_paired == 1:
        image = ops.pw_pack_weight_paired(_f32(w))
    else:
        image = ops.pw_pack_weight(_f32(w), wdt)
    rows = x.shape[0]
    y, buf = _guarded((1, rows, c_out), TORCH_DT[e.dout])
    bias = torch.zeros((c_out,), dtype=torch.float32, device=DEV)
    ops.pw_conv(x.view(1, rows, c_in), image, bias, N=1, rows_per_sample=rows, c_in=c_in, c_out=c_out, out_dtype=y.dtype, y=y,
                w_paired=w_paired, **kw)
    _guards_intact(buf, e.id)
    return _host(y.view(rows, c_out))


# ---- one launch recipe per entry id prefix: values (R, width) fp32 -> results (R, width) fp32
def _run_entry(e, values: np.ndarray) -> np.ndarray:
    nat, ops = _ops()
    R, Wd = values.shape
    x = _dev(values, e.din)
    act_code = {"gelu": nat.ACT_GELU, "sigmoid": nat.ACT_SIGMOID, "tanh": nat.ACT_TANH}
    i = e.id
    if i.startswith("gelu.fwd"):
        return _host(ops.gelu(x))
    if i.startswith("gelu.bwd"):
        return _host(ops.gelu(x, dy=_const(x.shape, 1.0, e.din)))
    if i.startswith("grn_bwd_apply"):
        A = torch.ones((1, Wd), dtype=torch.float32, device=DEV)
        B = torch.zeros((1, Wd), dtype=torch.float32, device=DEV)
        return _host(ops.grn_bwd_apply(_const((1, R, Wd), 1.0, e.din), x.view(1, R, Wd), A, B).view(R, Wd))
    if i.startswith("pw_conv.act"):
        code = act_code[i.split(".")[2]]
        if i.endswith(".stem"):
            y = _pw_conv(e, x, np.ones((8, 1)), c_in=1, c_out=8, act=code)
            assert all(np.array_equal(y[:, j].view(np.uint32), y[:, 0].view(np.uint32)) for j in range(8)), f"{i}: the 8 channels differ"
            return y[:, :1]
        if i.endswith(".head"):
            a = np.zeros((R, 8), dtype=np.float32)
            a[:, 0] = values[:, 0]
            w = np.zeros((1, 8))
            w[0, 0] = 1.0
            return _pw_conv(e, _dev(a, e.din), w, c_in=8, c_out=1, act=code)
        return _pw_conv(e, x, X.top_identity(Wd, Wd), c_in=Wd, c_out=Wd, act=code)
    if i.startswith("pw_conv.pre_act"):
        wp = {"generic": 0, "paired": 1, "rowmajor": 2}[i.split(".")[2]]
        c_out = 128 if Wd == 64 else Wd
        y = _pw_conv(e, x, X.top_identity(c_out, Wd), c_in=Wd, c_out=c_out, w_paired=wp, pre_act=nat.ACT_GELU)
        assert not y[:, Wd:].any(), f"{i}: the outputs behind the zero rows of W are not zero"
        return y[:, :Wd]
    if i.startswith("pw_conv.res_gelu_bwd"):
        wp = {"generic": 0, "paired": 1, "rowmajor": 2}[i.split(".")[2]]
        c_in = 64 if Wd == 128 else Wd
        ones = _const((R, c_in), 1.0, e.din)
        return _pw_conv(e, ones, X.zero_padded_identity(Wd, c_in), c_in=c_in, c_out=Wd, w_paired=wp, res=x.view(1, R, Wd),
                        res_mode=nat.RES_GELU_BWD)
    if i.startswith("linear_fwd"):
        c_out = 128 if Wd == 64 else Wd
        assert ops.linear_mfma_applies(x, Wd, c_out) == i.endswith(".mfma"), f"{i}: linear_mfma_applies says otherwise"
        y = _host(ops.linear_fwd(x, _f32(X.top_identity(c_out, Wd)), None, x_gelu=True))
        assert not y[:, Wd:].any()
        return y[:, :Wd]
    if i in ("linear_bwd.plain.f32", "linear_bwd.plain.bf16", "linear_bwd.mfma"):
        n = 64 if Wd == 128 else Wd                                    # dy (R, n), W (n, Wd): dx = (dy W) * g'(x)
        dy = _const((R, n), 1.0, e.din)
        assert ops.linear_mfma_applies(dy, n, Wd) == i.endswith(".mfma"), f"{i}: linear_mfma_applies says otherwise"
        dx, _, _, _ = ops.linear_bwd(dy, x, _f32(X.zero_padded_identity(n, Wd)), want_dx=True, want_w=False, x_gelu=True)
        return _host(dx)
    if i.startswith("pw_wgrad.") or i.startswith("linear_bwd.plain.dW"):
        out = np.empty_like(values)
        dy = _dev(np.eye(64, dtype=np.float32), e.din)
        knobs = dict(wgrad_valu=1) if ".valu" in i else {}
        with _knobs(**knobs):
            for r0 in range(0, R, 64):
                blk = x[r0:r0 + 64].contiguous()
                if i.startswith("linear_bwd.plain.dW"):
                    _, dW, _, _ = ops.linear_bwd(dy, blk, torch.zeros((64, Wd), dtype=torch.float32, device=DEV), want_dx=False, want_w=True,
                                                 x_gelu=True)
                else:
                    dW, _ = ops.pw_wgrad(blk.view(1, 64, Wd), dy.view(1, 64, 64), N=1, rows_per_sample=64, c_in=Wd, c_out=64, want_bias=False,
                                         x_act=nat.ACT_GELU)
                out[r0:r0 + 64] = _host(dW)
        return out
    if i.startswith("pw_mlp.train"):
        w2 = ops.pw_pack_weight_paired(_f32(X.top_identity(64, 32)))
        w3 = ops.pw_pack_weight_paired(_f32(X.top_identity(64, 32).T))
        ab = torch.stack([torch.ones(32), torch.zeros(32)]).view(1, 2, 32).to(DEV)
        b2, b3 = torch.zeros((64,), dtype=torch.float32, device=DEV), torch.zeros((32,), dtype=torch.float32, device=DEV)
        y, ybuf = _guarded((1, R, 32), torch.bfloat16)
        kw = dict(N=1, rows_per_sample=R, c_in=32, c_hid=64, c_out=32, y=y)
        if i.endswith(".stored"):
            hp, hbuf = _guarded((1, R, 64), torch.bfloat16)
            ops.pw_mlp(x.view(1, R, 32), ab, w2, b2, w3, b3, hidden_pre=hp, **kw)
            _guards_intact(hbuf, i + " hidden_pre")
            h = _host(hp.view(R, 64))
            keep = np.where(values == 0, np.float32(0), values)              # the expand GEMM's accumulator drops the sign of a zero
            assert np.array_equal(h[:, :32].view(np.uint32), keep.view(np.uint32)) and not h[:, 32:].any(), f"{i}: hidden_pre is not x beside zeros"
        else:
            ops.pw_mlp(x.view(1, R, 32), ab, w2, b2, w3, b3, train_nostore=True, **kw)
        _guards_intact(ybuf, i)
        return _host(y.view(R, 32))
    if i == "pw_mlp_bwd.d_hidden":
        dyv = np.zeros((R, 32), dtype=np.float32)
        dyv[:, 0] = 1.0                                                     # dy = e_0 in every row
        w3 = np.zeros((32, 64))
        w3[0, :] = 1.0                                                      # W3 (c_out, c_hid): first row ones -> (W3^T dy)[k] = 1
        w3t = ops.pw_pack_weight_paired(_f32(w3), transposed=True)
        w2t = ops.pw_pack_weight_paired(torch.zeros((64, 32), dtype=torch.float32, device=DEV), transposed=True)
        _, dh = ops.pw_mlp_bwd(_dev(dyv, "bf16").view(1, R, 32), x.view(1, R, 64), w3t, w2t, N=1, rows_per_sample=R, c_in=32, c_hid=64, c_out=32)
        return _host(dh.view(R, 64))
    if i.startswith("mixer_bwd_rc"):
        chid = int(i.split(".")[1])
        assert ops.mixer_bwd_rc_supported(32, chid, 32, torch.bfloat16) == 2
        out = np.empty_like(values)
        dy = _dev(np.eye(32, dtype=np.float32), "bf16").view(1, 32, 32)
        ab = torch.stack([torch.ones(32), torch.zeros(32)]).view(1, 2, 32).to(DEV)
        w2 = ops.pw_pack_weight_paired(_f32(X.zero_padded_identity(chid, 32)))
        w3t = ops.pw_pack_weight_paired(torch.ones((32, chid), dtype=torch.float32, device=DEV), transposed=True)
        b2 = torch.zeros((chid,), dtype=torch.float32, device=DEV)
        for r0 in range(0, R, 32):
            dW3, _, dhp = ops.mixer_bwd_rc(x[r0:r0 + 32].contiguous().view(1, 32, 32), ab, dy, w2, b2, w3t, N=1, rows_per_sample=32, c=32, c_hid=chid,
                                           c_out=32, want_bias=False)
            full = _host(dW3) if i.endswith(".dW3") else _host(dhp.view(32, chid))
            for g in range(32, chid, 32):
                assert np.array_equal(full[:, g:g + 32].view(np.uint32), full[:, :32].view(np.uint32)), f"{i}: the hidden-channel groups differ"
            out[r0:r0 + 32] = full[:, :32]
        return out
    if i.startswith("pw_wgrad_dgrad"):
        assert ops.pw_wgrad_dgrad_supported(Wd, 32, torch.bfloat16)
        out = np.empty_like(values)
        dy = _dev(np.eye(32, dtype=np.float32), "bf16").view(1, 32, 32)
        wt = ops.pw_pack_weight_paired(torch.ones((32, Wd), dtype=torch.float32, device=DEV), transposed=True)
        for r0 in range(0, R, 32):
            dW, _, dhp = ops.pw_wgrad_dgrad(x[r0:r0 + 32].contiguous().view(1, 32, Wd), dy, wt, N=1, rows_per_sample=32, c_in=Wd, c_out=32,
                                            want_bias=False)
            out[r0:r0 + 32] = _host(dW) if i.endswith(".dW") else _host(dhp.view(32, Wd))
        return out
    raise AssertionError(f"no launch for {i}")


def _report(line: str):
    path = os.environ.get("PYTC_ACT_DOMAIN_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _check_classes(e, x, got):
    """the class rules on the inputs this entry keeps (non-finite ones are swept as 0 where they would share a sum)"""
    fin, nan = np.isfinite(x), np.isnan(x)
    assert np.isfinite(got[fin]).all(), f"{e.id}: a finite input gave NaN / inf"
    assert np.isnan(got[nan]).all(), f"{e.id}: NaN in did not give NaN out"
    zero = fin & (x == 0)
    if e.fn in ("gelu_erf", "gelu_fast"):
        assert (got[zero] == 0).all(), f"{e.id}: f(+-0) != 0"
        if not e.spec.zero_sign_lost:
            assert np.array_equal(np.signbit(got[zero]), np.signbit(x[zero])), f"{e.id}: +-0 in did not give +-0 out"
    elif e.fn in ("gelu_erf_grad", "gelu_fast_grad", "gelu_grad_libm"):
        assert (got[zero] == np.float32(0.5)).all(), f"{e.id}: g'(+-0) is not exactly 1/2"
    elif e.fn == "sigmoid":
        assert (got[zero] == np.float32(0.5)).all()
    elif e.fn == "tanh":
        assert (got[zero] == 0).all()


@pytest.mark.parametrize("e", X.ENTRIES, ids=[e.id for e in X.ENTRIES])
def test_entry_point_inside_its_interval(e):
    for sweep in e.sweep:
        x = X.sweep_values(e, sweep)
        with _knobs(**KNOB_DEFAULTS):
            got = _run_entry(e, x)
            again = _run_entry(e, x)
        assert got.shape == x.shape
        same = (got.view(np.uint32) == again.view(np.uint32)) | (np.isnan(got) & np.isnan(again))
        assert same.all(), f"{e.id} [{sweep}]: a second launch gave other bits at {int((~same).sum())} inputs"
        iv = X.expected(e, x)
        ok = X.inside(iv, got)
        pos = X.position(iv, got)
        ndiff, worst = X.against_central(e.fn, x, got, mid=e.mid, out=e.dout)
        line = (f"{e.id:36s} {sweep:9s} {e.fn:15s} worst position in [lo, hi] {pos:.3f} of the half-width; differs from the un-nudged model at "
                f"{ndiff} of {x.size} inputs, by at most {worst:.3e}")
        print(line)
        _report(line)
        assert ok.all(), X.describe_failures(f"{e.id} [{sweep}]", x, got, iv, ~ok)
        _check_classes(e, x, got)
        _RESULTS[(e.id, sweep)] = (got, np.isfinite(x))


def _groups():
    g = {}
    for e in X.ENTRIES:
        g.setdefault(e.group, []).append(e)
    return [v for v in g.values() if len(v) > 1]


@pytest.mark.parametrize("members", _groups(), ids=["+".join(e.id for e in m)[:120] for m in _groups()])
def test_same_function_same_bits(members):
    """entry points filed under the same function, input type and rounding: identical bits on every finite input, no tolerance"""
    for sweep in ("bf16_all", "f32_grid"):
        have = []
        for e in members:
            if sweep not in e.sweep:
                continue
            if (e.id, sweep) not in _RESULTS:
                with _knobs(**KNOB_DEFAULTS):
                    x = X.sweep_values(e, sweep)
                    _RESULTS[(e.id, sweep)] = (_run_entry(e, x), np.isfinite(x))
            have.append(e)
        if len(have) < 2:
            continue
        first = have[0]
        a, fa = _RESULTS[(first.id, sweep)]
        for e in have[1:]:
            b, fb = _RESULTS[(e.id, sweep)]
            both = (fa.ravel() & fb.ravel())
            av, bv = a.ravel().copy(), b.ravel().copy()
            if first.spec.zero_sign_lost or e.spec.zero_sign_lost:          # 0 + -0 = +0 in an accumulator: compare zeros without sign
                av[av == 0] = 0.0
                bv[bv == 0] = 0.0
            diff = both & (av.view(np.uint32) != bv.view(np.uint32))
            if diff.any():
                k = int(np.flatnonzero(diff)[0])
                xs = X.sweep_values(first, sweep).ravel()
                raise AssertionError(f"{first.id} and {e.id} [{sweep}] are filed under {first.fn} but differ at {int(diff.sum())} inputs, first x = "
                                     f"{xs[k]!r} (bits 0x{int(xs[k:k + 1].view(np.uint32)[0]):08x}): {av[k]!r} vs {bv[k]!r}")


def test_gelu_fast_grad_non_finite_classes():
    """the swept entries of gelu_fast_with_grad's derivative (pw_wgrad_dgrad at C_in = 128, mixer_bwd_rc) share sums with their weight
    gradients, so the main sweep replaces non-finite inputs by 0.  One more pw_wgrad_dgrad launch with the 256 non-finite patterns in
    (dhp only: it is elementwise in hp)"""
    e = X.BY_ID["pw_wgrad_dgrad.128.dhp"]
    b = X.bf16_all().ravel()
    x = np.zeros((32, 128), dtype=np.float32)
    x.ravel()[:256] = b[~np.isfinite(b)]
    got = _run_entry(e, x)
    iv = X.interval(e.fn, x, out="bf16")
    ok = X.inside(iv, got)
    assert ok.all(), X.describe_failures(e.id + " [non-finite]", x, got, iv, ~ok)
    assert np.isnan(got[np.isnan(x)]).all()

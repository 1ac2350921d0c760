"""The per-row LayerNorm forward and dx of all three forms (layernorm_wide_*, layernorm_any_*, layernorm_rows_*) on the rows of
tests/layernorm_exact_cases.py: rows mu + a sigma with eps = 0, whose y, dx, dgamma and dbeta are exact in fp32 in any summation order,
compared with equality; and integer rows with eps = 1e-5 against fp64 within the per-element bound derived in
layernorm_exact_cases.general_bounds.

layernorm_rows_* (1.0f / sqrtf) is always held to equality.  For layernorm_wide_* / layernorm_any_* the module first asks the device
whether rsqrtf returns 2^-k at 4^k; where it does (the MI355X does: profiles/layernorm_exact_probe.txt) fp32 is held to equality too,
otherwise to layernorm_exact_cases.rsqrt_bound.  bf16 outputs are compared with equality either way.  Every output sits inside a
NaN-filled guarded buffer, every operand inside a NaN-filled buffer, and a second launch through hip_ops repeats the bits."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import layernorm_exact_cases as X  # noqa: E402
from test_gpu_pw_conv_exact import _bits, _guarded, _guards_intact  # noqa: E402  (the guard-band helpers of the pw-conv suite)

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ops():
    from pytorch_connectomics_amd import _native as nat, hip_ops as ops
    return nat, ops


_RSQRT_EXACT = {}


def rsqrt_exact(form: str) -> bool:
    """does the form's reciprocal square root return 1 / a at a^2, a = 1, 2, 4, 8?  (xhat of a +-a row is then +-1)"""
    if form not in _RSQRT_EXACT:
        _, ops = _ops()
        ok = True
        for a in (1.0, 2.0, 4.0, 8.0):
            x = torch.tensor([[a, -a] * 32], dtype=torch.float32, device=DEV)
            if form == "wide":
                y = ops.layernorm_wide(x, torch.ones(64, device=DEV), torch.zeros(64, device=DEV), 0.0)
            else:
                y = ops.layernorm_any(x, None, None, 0.0)
            ok = ok and bool((y.abs() == 1.0).all())
        _RSQRT_EXACT[form] = ok
    return _RSQRT_EXACT[form]


def _put(a, t):
    if a is None:
        return None, None
    return _guarded(a.shape, t, X.to_storage(a, "f32" if t == torch.float32 else "bf16").to(DEV))


def _launch(c, x, dy, gamma, beta, eps):
    """forward and backward through the C entry points, as hip_ops calls them -> (y, dx, dgamma, dbeta) with y, dx guarded"""
    nat, ops = _ops()
    lib, p, st = nat.lib(), ops._p, ops._stream()
    code = ops.dtype_code(x.dtype)
    rows, C = x.shape
    y, ybuf = _guarded((rows, C), x.dtype)
    dx, dxbuf = _guarded((rows, C), x.dtype)
    f32 = dict(dtype=torch.float32, device=DEV)
    dg = db = None
    if c.form == "wide":
        nat.check(lib.pytc_layernorm_wide(p(x), p(y), p(gamma), p(beta), rows, C, eps, code, st), c.id)
        part = torch.empty((int(lib.pytc_layernorm_wide_bwd_slots(rows)), 2, C), **f32)
        dg, db = torch.empty((C,), **f32), torch.empty((C,), **f32)
        nat.check(lib.pytc_layernorm_wide_bwd(p(dy), p(x), p(gamma), p(dx), p(part), p(dg), p(db), rows, C, eps, code, st), c.id)
    elif c.form == "any":
        nat.check(lib.pytc_layernorm_any(p(x), p(y), p(gamma), p(beta), rows, C, eps, code, st), c.id)
        stats = part = None
        if gamma is not None:
            stats = torch.empty((rows, 2), **f32)
            part = torch.empty((int(lib.pytc_layernorm_any_bwd_slots(rows)), 2, C), **f32)
            dg, db = torch.empty((C,), **f32), torch.empty((C,), **f32)
        nat.check(lib.pytc_layernorm_any_bwd(p(dy), p(x), p(gamma), p(dx), p(stats), p(part), p(dg), p(db), rows, C, eps, code, st), c.id)
    else:
        nat.check(lib.pytc_layernorm_rows(p(x), p(y), p(gamma), p(beta), rows, C, eps, code, st), c.id)
        slots = int(lib.pytc_layernorm_rows_bwd_slots(rows, C, code))
        assert slots == min(X.ROWS_BWD_MAX_BLOCKS, -(-rows // X.rows_rpb(C)))
        part = torch.full((slots, 2, C), float("nan"), **f32)
        nat.check(lib.pytc_layernorm_rows_bwd(p(dy), p(x), p(gamma), p(dx), p(part), rows, C, eps, code, st), c.id)
        torch.cuda.synchronize()
        db, dg = part[:, 0].double().sum(0), part[:, 1].double().sum(0)        # integer partials on the exact rows: any order
    torch.cuda.synchronize()
    _guards_intact(ybuf, f"{c.id} y")
    _guards_intact(dxbuf, f"{c.id} dx")
    return y, dx, dg, db


def _through_ops(c, x, dy, gamma, beta, eps):
    _, ops = _ops()
    if c.form == "wide":
        return ops.layernorm_wide(x, gamma, beta, eps), ops.layernorm_wide_bwd(dy, x, gamma, eps)[0]
    if c.form == "any":
        return ops.layernorm_any(x, gamma, beta, eps), ops.layernorm_any_bwd(dy, x, gamma, eps)[0]
    return ops.layernorm_rows(x, gamma, beta, eps), ops.layernorm_rows_bwd(dy, x, gamma, eps)[0]


def _held(got, want64, bound, what):
    """|got - want| <= bound per element, nothing unwritten -> the largest error over its bound"""
    g = got.double().cpu().numpy()
    assert not np.isnan(g).any(), f"{what}: {int(np.isnan(g).sum())} elements were never written"
    ratio = np.abs(g - want64) / np.maximum(bound, 1e-300)
    worst = float(ratio.max())
    assert worst <= 1.0, f"{what}: error over the derived bound {worst:.3g} at {np.unravel_index(ratio.argmax(), ratio.shape)}"
    return worst


def _equal(got, want64, dt, what):
    want = X.to_storage(want64, dt)
    g = got.cpu()
    nan = int(torch.isnan(g.float()).sum())
    assert nan == 0, f"{what}: {nan} of {g.numel()} elements were never written"
    bad = (g != want).nonzero()
    assert len(bad) == 0, (f"{what}: {len(bad)} of {g.numel()} elements differ from the exact answer; first (row, c), got, want: "
                           f"{[(tuple(i.tolist()), float(g[tuple(i)]), float(want[tuple(i)])) for i in bad[:6]]}")


@pytest.mark.parametrize("c", X.cases(), ids=X.ids(X.cases()))
def test_layernorm_forward_and_dx(c):
    dt = X.TORCH_DT[c.dt]
    gamma64, beta64 = X.affine(c)
    gamma, gbuf = _put(gamma64, torch.float32)
    beta, bbuf = _put(beta64, torch.float32)
    exact = c.form == "rows" or c.dt == "bf16" or rsqrt_exact(c.form)
    # ---- the rows with an exact answer
    d = X.exact_rows(c)
    x, xbuf = _put(d["x"], dt)
    dy, dybuf = _put(d["dy"], dt)
    y, dx, dg, db = _launch(c, x, dy, gamma, beta, d["eps"])
    worst = 0.0
    if exact:
        _equal(y, d["y"], c.dt, f"{c.id} exact rows y")
        _equal(dx, d["dx"], c.dt, f"{c.id} exact rows dx")
    else:
        by, bdx = X.rsqrt_bound(c, d)
        worst = max(_held(y, d["y"], by, f"{c.id} exact rows y"), _held(dx, d["dx"], bdx, f"{c.id} exact rows dx"))
    if dg is not None and (exact or c.form == "rows"):
        assert np.array_equal(dg.double().cpu().numpy(), d["dgamma"]), f"{c.id}: dgamma of the exact rows is not the integer sum"
    if db is not None:
        assert np.array_equal(db.double().cpu().numpy(), d["dbeta"]), f"{c.id}: dbeta of the exact rows is not the integer sum"
    y2, dx2 = _through_ops(c, x, dy, gamma, beta, d["eps"])
    torch.cuda.synchronize()
    assert torch.equal(_bits(y2), _bits(y)) and torch.equal(_bits(dx2), _bits(dx)), f"{c.id}: hip_ops / a second run differs"
    # ---- general rows against fp64 within the derived bound
    gd = X.general_rows(c)
    y64, dx64, By, Bdx = X.general_bounds(c, gd)
    xg, xgbuf = _put(gd["x"], dt)
    dyg, dygbuf = _put(gd["dy"], dt)
    yg, dxg, _, dbg = _launch(c, xg, dyg, gamma, beta, gd["eps"])
    wy, wdx = _held(yg, y64, By, f"{c.id} general rows y"), _held(dxg, dx64, Bdx, f"{c.id} general rows dx")
    if dbg is not None:
        assert np.array_equal(dbg.double().cpu().numpy(), gd["dy"].sum(0)), f"{c.id}: dbeta of the general rows"
    for b in (gbuf, bbuf, xbuf, dybuf, xgbuf, dygbuf):
        if b is not None:
            _guards_intact(b, f"{c.id} operand")
    print(f"LNPROBE {c.id} exact-rows {'equality' if exact else f'rsqrt-bound {worst:.3g}'} general y {wy:.3g} dx {wdx:.3g} of the bound")


def test_rows_forward_past_the_block_cap():
    """262 145 rows of C = 512 in bf16: 65 537 row blocks against the 65 536-block cap, so block 0 takes a second trip.  Every row is
    the same two-level row; the expected tensor is a broadcast, compared on the device."""
    nat, ops = _ops()
    c = X.fwd_cap_case()
    assert -(-c.rows // X.rows_rpb(c.C)) == X.ROWS_FWD_MAX_BLOCKS + 1
    one = X.LnCase("rows", "bf16", c.C, 1)
    d = X.exact_rows(one)
    gamma64, beta64 = X.affine(one)
    gamma, beta = _put(gamma64, torch.float32)[0], _put(beta64, torch.float32)[0]
    x, xbuf = _guarded((c.rows, c.C), torch.bfloat16)
    x.copy_(X.to_storage(d["x"], "bf16").to(DEV).expand(c.rows, c.C))
    y, ybuf = _guarded((c.rows, c.C), torch.bfloat16)
    nat.check(nat.lib().pytc_layernorm_rows(ops._p(x), ops._p(y), ops._p(gamma), ops._p(beta), c.rows, c.C, 0.0, ops.dtype_code(x.dtype),
                                            ops._stream()), c.id)
    torch.cuda.synchronize()
    _guards_intact(ybuf, c.id)
    want = X.to_storage(d["y"], "bf16").to(DEV)
    bad = int((_bits(y) != _bits(want.expand(c.rows, c.C))).sum())
    assert bad == 0, f"{c.id}: {bad} of {y.numel()} outputs differ from the row's exact answer (NaN: never written)"
    _guards_intact(xbuf, c.id + " operand")


def test_rows_form_refuses_by_name_what_it_cannot_split():
    _, ops = _ops()
    for C in X.ROWS_REFUSED:
        assert X.ln_vec(C) == 0
        x = torch.ones((4, C), dtype=torch.float32, device=DEV)
        y_before = None
        with pytest.raises(RuntimeError) as err:
            y_before = ops.layernorm_rows(x, None, None, 1e-5)
        assert "layernorm_rows" in str(err.value) and f"C={C}" in str(err.value) and y_before is None
        with pytest.raises((RuntimeError, ValueError)) as err:
            ops.layernorm_rows_bwd(x, x, None, 1e-5)
        assert "layernorm_rows_bwd" in str(err.value) and str(C) in str(err.value)
    for C in X.ROWS_C:
        assert X.ln_vec(C) > 0
    torch.cuda.synchronize()


def test_row_tile_limits_of_linear_and_layernorm_any_refuse_by_name():
    """linear_launch has its M tiles and layernorm_any_param_kernel its row slots on gridDim.y: one past 65535 is refused with the
    limit in the message, before anything is launched (the buffers are allocated, never initialised or read)."""
    nat, ops = _ops()
    lib, p, st = nat.lib(), ops._p, ops._stream()
    M = 65535 * 64 + 1
    x = torch.empty((M, 1), dtype=torch.bfloat16, device=DEV)
    w = torch.zeros((1, 1), dtype=torch.float32, device=DEV)
    y = torch.empty((M, 1), dtype=torch.bfloat16, device=DEV)
    for name, call in (("linear_fwd", lambda: lib.pytc_linear_fwd(p(x), p(w), None, None, 0, None, p(y), M, 1, 1, 0, nat.BF16, st)),
                       ("linear_bwd_data", lambda: lib.pytc_linear_bwd_data(p(x), p(w), None, p(y), M, 1, 1, nat.BF16, st))):
        with pytest.raises(RuntimeError) as err:
            nat.check(call(), name)
        assert name in str(err.value) and "65535" in str(err.value) and str(M) in str(err.value), str(err.value)
    rows = 65535 * 256 + 1
    xs = torch.empty((rows, 16), dtype=torch.bfloat16, device=DEV)
    g = torch.ones(16, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError) as err:
        ops.layernorm_any_bwd(xs, xs, g, 1e-5)
    assert "layernorm_any_bwd" in str(err.value) and "65535" in str(err.value) and str(rows) in str(err.value), str(err.value)
    torch.cuda.synchronize()

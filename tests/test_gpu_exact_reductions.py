"""Split-slot reductions at production training sizes with exact-arithmetic operands (tests/exact_reduction_cases.py): ternary bf16
values, exact norm affines and GELU operands in {0, 16} make every partial sum exact in fp32, so each weight / bias gradient, channel
statistic and LayerNorm dbeta must equal its fp64 reference bit for bit, in every kernel form a tuning knob selects, on a second run,
and through the deferred (one-launch) slot reduction.  A lost, doubled or misrouted row or slot is a nonzero integer difference.
LayerNorm dgamma (x-hat is not exact) is held to the derived bound (L + S + 2) 2^-24 sum|t| instead, on operands whose last slot
moves the result by more than twice that bound.  The GroupNorm forms take exact statistics (mean in {-1, 0, 1}, rstd a power of two),
so their x-hat, dW2 / db2 and norm sums are exact too.

Case IDs carry the slot count from the Python mirrors of the dispatchers (exact_reduction_cases.py); the case asserts it is > 1 and equal
to the library's count.  The dense-conv and statistic-slot cases have no mirror: their IDs name the shape, and the case asserts the
library's count is > 1.  The deferred reduction, the second run and the knob forms are checked where the library has them: pw / dw /
mixer deferred and knob forms, conv3d's matrix-core knob, the fused / unfused projecting-conv forms."""
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import exact_reduction_cases as X  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ops():
    from pytorch_connectomics_amd import _native as nat, hip_ops as ops
    return nat, ops


def _same(got: torch.Tensor, want64: torch.Tensor, what: str) -> None:
    """bit equality of an fp32 result with the exact fp64 sum (both are integers / dyadics far inside fp32's exact range)."""
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want64.shape), f"{what}: {got.dtype} {tuple(got.shape)}"
    d = (got.double() - want64).abs()
    assert float(d.max()) == 0.0, f"{what}: {int((d != 0).sum())} outputs off, max |diff| {float(d.max())} (exact inputs: must be 0)"


class _Knobs:
    """set tuning knobs for a block, restore the library defaults afterwards"""
    DEFAULTS = {"wgrad_valu": 0, "wgrad_small_split": 1, "wgrad_whole_rounds": 1, "dw_wgrad_march": 1, "dw_wgrad_vec": 1,
                "conv_wgrad_mfma": 1, "mixer_bwd_rc_slot_div": 1, "wgrad_dgrad_fused": 1}

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        _, ops = _ops()
        for k, v in self.kv.items():
            ops.set_tuning(k, int(v))

    def __exit__(self, *exc):
        _, ops = _ops()
        for k in self.kv:
            ops.set_tuning(k, self.DEFAULTS[k])
        return False


def _conv_wgrad_ref(small, big, kernel, stride, pad, depthwise=False):
    """fp64 sum_r small[r][o] * big[r * stride + tap - pad][k] (zeros outside big) -> (C_o, C_k, *kernel), or (taps, C) depthwise."""
    N, d, h, w, co = small.shape
    ck = big.shape[-1]
    dims = (d, h, w)
    lp = [int(p) for p in pad]
    rp = [max(0, stride[i] * (dims[i] - 1) + kernel[i] - lp[i] - big.shape[1 + i]) for i in range(3)]
    bp = F.pad(big.double(), (0, 0, lp[2], rp[2], lp[1], rp[1], lp[0], rp[0]))
    s = small.double().reshape(-1, co)
    out = []
    for kz in range(kernel[0]):
        for ky in range(kernel[1]):
            for kx in range(kernel[2]):
                sl = bp[:, kz:kz + stride[0] * (d - 1) + 1:stride[0], ky:ky + stride[1] * (h - 1) + 1:stride[1],
                        kx:kx + stride[2] * (w - 1) + 1:stride[2]].reshape(-1, ck)
                out.append((s * sl).sum(0) if depthwise else s.t() @ sl)
                del sl
    if depthwise:
        return torch.stack(out)
    return torch.stack(out, -1).view(co, ck, *kernel)


# ------------------------------------------------------------------------------------------------ pointwise weight gradients
def _pw_id(c):
    f = X.split_facts(c.rows, c.N, c.slots)
    return f"{c.name}-slots{c.slots}" + ("-ragged" if f["ragged"] else "") + ("-straddle" if f["straddle"] else "")


def _pw_operands(c, seed):
    nat, _ = _ops()
    if c.gelu:
        x = X.binary((c.N, c.rows, c.c_in), c.density_x, seed, value=16.0, device=DEV)
        xn = x.double()                                     # gelu(0) = 0, gelu(16) = 16 exactly (host test: every GELU form)
    else:
        x = X.ternary((c.N, c.rows, c.c_in), c.density_x, seed, device=DEV)
        xn = x.double()
    ab = None
    if c.ab:
        ab = X.exact_affine(c.N, c.c_in, seed + 7).to(DEV)
        xn = xn * ab[:, 0].double()[:, None] + ab[:, 1].double()[:, None]
    dy = X.ternary((c.N, c.rows, c.c_out), c.density_dy, seed + 1, device=DEV)
    return x, ab, dy, xn, (nat.ACT_GELU if c.gelu else nat.ACT_NONE)


@pytest.mark.parametrize("c", X.pw_cases(), ids=_pw_id)
def test_pw_wgrad_exact_at_training_sizes(c):
    nat, ops = _ops()
    assert c.slots > 1
    x, ab, dy, xn, act = _pw_operands(c, seed=c.rows + c.c_in)
    dyd = dy.double().reshape(-1, c.c_out)
    colsum = dyd.abs().sum(0)
    bound, quantum = X.pw_case_abs_bound(c)
    X.assert_exact_cap(X.gemm_abs_bound(float(xn.abs().max()), colsum), quantum, what=c.name)
    assert float(colsum.max()) < X.EXACT_F32
    want = dyd.t() @ xn.reshape(-1, c.c_in)
    want_b = dyd.sum(0)
    # the last slot carries signal: losing it (or doubling it) changes dW
    a0, b0 = X.split_facts(c.rows, c.N, c.slots)["last"]
    assert float((dyd[a0:b0].t() @ xn.reshape(-1, c.c_in)[a0:b0]).abs().max()) > 0
    del xn
    kw = dict(N=c.N, rows_per_sample=c.rows, c_in=c.c_in, c_out=c.c_out, ab=ab, x_act=act)
    dW, db = ops.pw_wgrad(x, dy, **kw)
    _same(dW, want, "dW")
    _same(db, want_b, "db")
    dr = ops.DeferredReduce()
    dW2, db2 = ops.pw_wgrad(x, dy, defer=dr, **kw)
    used = dr.items[0][3]
    dr.flush()
    assert used == c.slots, f"the library split into {used} slots, the mirror says {c.slots}"
    _same(dW2, want, "deferred dW")
    _same(db2, want_b, "deferred db")
    dW3, db3 = ops.pw_wgrad(x, dy, **kw)
    assert torch.equal(dW3, dW) and torch.equal(db3, db)                  # run to run
    for knobs in ({"wgrad_valu": 1}, {"wgrad_small_split": 0}, {"wgrad_whole_rounds": 0}):
        with _Knobs(**knobs):
            dWk, dbk = ops.pw_wgrad(x, dy, **kw)
        assert torch.equal(dWk, dW) and torch.equal(dbk, db), f"form {knobs} differs"


PWD_CASES = [X.PwCase("L0_project_64x32", 4, 112 ** 3, 64, 32, gelu=True),
             X.PwCase("L0_up_project_128x32", 4, 112 ** 3, 128, 32, gelu=True),
             X.PwCase("L0_project_32x32", 4, 112 ** 3, 32, 32, gelu=True),
             X.PwCase("odd_N5_16x80x48_project_64x32", 5, 16 * 80 * 48, 64, 32, gelu=True),
             X.PwCase("odd_N3_33x47x61_project_64x32", 3, 33 * 47 * 61, 64, 32, gelu=True)]      # 94 611 rows per sample: rows % 32 = 19


@pytest.mark.parametrize("c", PWD_CASES, ids=_pw_id)
def test_pw_wgrad_dgrad_weight_part_exact(c):
    """The fused weight + data gradient of a mixer's projecting conv: its dW / db are the pw_wgrad(x_act=GELU) sums, exactly, and its
    data gradient is dhp = (dy . W) * gelu'(hp), exactly: dy and W are ternary, so a row of dy . W is an integer of magnitude <= C_out = 32,
    and hp in {0, 16} makes gelu' exactly 1/2 and 1 (test_mixer_bwd_rc_exact) -- every dhp is a multiple of 1/2 below 2^6,
    a bf16 number."""
    nat, ops = _ops()
    if not ops.pw_wgrad_dgrad_supported(c.c_in, c.c_out, torch.bfloat16):
        pytest.fail(f"pw_wgrad_dgrad does not cover {c.c_in} -> {c.c_out}")
    hp, _, dy, xn, _ = _pw_operands(c, seed=c.rows + 3 * c.c_in)
    dyd = dy.double().reshape(-1, c.c_out)
    X.assert_exact_cap(X.gemm_abs_bound(16.0, dyd.abs().sum(0)), 16.0, what=c.name)
    want = dyd.t() @ xn.reshape(-1, c.c_in)
    del xn
    w = X.ternary((c.c_out, c.c_in), 0.5, 11, dtype=torch.float32, device=DEV)
    wtp = ops.packed_paired(w, transposed=True)
    dr = ops.DeferredReduce()
    dW, db, dhp = ops.pw_wgrad_dgrad(hp, dy, wtp, N=c.N, rows_per_sample=c.rows, c_in=c.c_in, c_out=c.c_out, defer=dr)
    used = dr.items[0][3]
    dr.flush()
    assert used == c.slots > 1
    _same(dW, want, "dW")
    _same(db, dyd.sum(0), "db")
    assert tuple(dhp.shape) == (c.N, c.rows, c.c_in) and dhp.dtype == torch.bfloat16
    for n in range(c.N):                                    # a sample at a time: integer sums of <= 32 ternary products, exact in fp32
        want_dhp = (dy[n].float() @ w) * torch.where(hp[n] == 16.0, 1.0, 0.5)
        assert float(want_dhp.abs().max()) <= c.c_out
        bad = int((dhp[n].float() != want_dhp).sum())
        assert bad == 0, f"dhp: {bad} of {want_dhp.numel()} elements of sample {n} differ from (dy . W) gelu'(hp)"
    del want_dhp
    dW2, db2, dhp2 = ops.pw_wgrad_dgrad(hp, dy, wtp, N=c.N, rows_per_sample=c.rows, c_in=c.c_in, c_out=c.c_out)
    assert torch.equal(dW2, dW) and torch.equal(db2, db) and torch.equal(dhp2, dhp)
    with _Knobs(wgrad_dgrad_fused=0):                       # the unfused form the caller then takes: pw_wgrad(x_act=GELU)
        assert not ops.pw_wgrad_dgrad_supported(c.c_in, c.c_out, torch.bfloat16)
        dWu, dbu = ops.pw_wgrad(hp, dy, N=c.N, rows_per_sample=c.rows, c_in=c.c_in, c_out=c.c_out, x_act=nat.ACT_GELU)
    _same(dWu, want, "unfused dW")
    _same(dbu, dyd.sum(0), "unfused db")


# ------------------------------------------------------------------------------------------------ depthwise weight gradients
def _dw_id(c):
    forms = sorted({X.dw_wgrad_form(c.gdims, c.xdims, c.C, 3, c.stride, march=m, vec=v) for m, v in ((1, 1), (0, 1), (0, 0))})
    return f"{c.name}-{'+'.join(forms)}-slots{X.dw_wgrad_slots(c.N, c.gdims, c.xdims, c.C, 3, c.stride)}"


@pytest.mark.parametrize("c", X.dw_cases(), ids=_dw_id)
def test_dw_wgrad_exact_at_training_sizes(c):
    """The depthwise weight gradient of the stride-1 block, the stride-2 down block and the transposed up block (training/autograd.py
    _dw_backward call shapes) in every form the dispatcher has for the shape (z-march, 16-byte vector, generic)."""
    nat, ops = _ops()
    g = X.ternary((c.N, *c.gdims, c.C), 0.5, c.C + c.gdims[0], device=DEV)
    x = X.ternary((c.N, *c.xdims, c.C), 0.5, c.C + c.xdims[0] + 1, device=DEV)
    per_out = c.N * c.gdims[0] * c.gdims[1] * c.gdims[2]
    X.assert_exact_cap(per_out, 1.0, what=c.name)                           # |g x| <= 1 per position
    want = _conv_wgrad_ref(g, x, (3, 3, 3), (c.stride,) * 3, (1, 1, 1), depthwise=True)
    want_b = g.double().reshape(-1, c.C).sum(0)
    want_b = want_b if c.kind != "up" else None
    i3 = ops._i3
    results = []
    for march, vec in ((1, 1), (0, 1), (0, 0)):
        form = X.dw_wgrad_form(c.gdims, c.xdims, c.C, 3, c.stride, march=bool(march), vec=bool(vec))
        if results and form == results[-1][0]:
            continue
        with _Knobs(dw_wgrad_march=march, dw_wgrad_vec=vec):
            slots = nat.lib().pytc_dw_wgrad_slots(c.N, i3(c.gdims), i3(c.xdims), c.C, 3, c.stride, nat.BF16)
            mirror = X.dw_wgrad_slots(c.N, c.gdims, c.xdims, c.C, 3, c.stride, march=bool(march), vec=bool(vec))
            assert slots == mirror > 1, f"{form}: library {slots} slots, mirror {mirror}"
            dW, db = ops.dw_wgrad(g, x, K=3, stride=c.stride, want_bias=want_b is not None)
            dr = ops.DeferredReduce()
            dWd, dbd = ops.dw_wgrad(g, x, K=3, stride=c.stride, want_bias=want_b is not None, defer=dr, channel_major=True)
            assert dr.items[0][3] == slots
            dr.flush()
        _same(dW, want, f"{form} dW")
        _same(dWd, want.t(), f"{form} deferred (channel-major) dW")
        if want_b is not None:
            _same(db, want_b, f"{form} db")
            _same(dbd, want_b, f"{form} deferred db")
        results.append((form, dW, db))
    dW2, _ = ops.dw_wgrad(g, x, K=3, stride=c.stride, want_bias=False)
    assert torch.equal(dW2, results[0][1])                                  # run to run


# ------------------------------------------------------------------------------------------------ channel statistics
STATS_CASES = [(4, 112 ** 3, 32), (4, 112 ** 3, 64), (4, 28 ** 3, 128), (4, 7 ** 3, 512), (3, 32 * 48 * 64, 32), (5, 16 * 80 * 48, 64)]


@pytest.mark.parametrize("N,rows,C", STATS_CASES,
                         ids=[f"N{n}_rows{r}_C{c}-slots{X.colstats_slots(r)}" for n, r, c in STATS_CASES])
def test_channel_stats_slot_partials_exact(N, rows, C):
    """Every (sample, slot) partial (sum x, sum x^2) of pytc_channel_stats equals the fp64 sum over exactly that slot's rows."""
    nat, ops = _ops()
    slots = X.colstats_slots(rows)
    assert nat.lib().pytc_channel_stats_slots(rows) == slots > 1
    x = X.ternary((N, rows, C), 0.5, rows + C, device=DEV)
    X.assert_exact_cap(rows, 1.0)
    st = ops.channel_stats(x)
    assert tuple(st.shape) == (N, slots, 2, C)
    xd = x.double()
    rps = -(-rows // slots)
    pad = rps * slots - rows
    xs = F.pad(xd, (0, 0, 0, pad)).view(N, slots, rps, C)
    want = torch.stack([xs.sum(2), (xs * xs).sum(2)], 2)
    _same(st, want, "channel_stats")
    assert torch.equal(ops.channel_stats(x), st)


# ------------------------------------------------------------------------------------------------ dense conv weight gradients
CONV_CASES = [("rsunet_stock_L0_k333", 2, (18, 160, 160), 24, 24, (3, 3, 3)),
              ("rsunet_stock_L0_k133", 2, (18, 160, 160), 24, 24, (1, 3, 3)),
              ("rsunet_stock_L2_k333", 2, (18, 40, 40), 48, 48, (3, 3, 3)),
              ("monai_c5_L0_k333", 1, (24, 256, 256), 32, 32, (3, 3, 3)),
              ("monai_c5_L3_k333", 1, (3, 32, 32), 256, 256, (3, 3, 3))]


@pytest.mark.parametrize("name,N,dims,ci,co,k", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv3d_wgrad_exact(name, N, dims, ci, co, k):
    nat, ops = _ops()
    ws = nat.lib().pytc_conv3d_wgrad_ws_elems(N, *dims, ci, co, ops._i3(k), nat.BF16)
    slots = ws // (k[0] * k[1] * k[2] * ci * co)
    print(f"[{name}] slots {slots}")
    assert slots > 1                                     # (the plan's slot count: the workspace holds exactly slots x taps x C_out x C_in)
    a = X.ternary((N, *dims, ci), 0.5, ci + dims[1], device=DEV)
    dy = X.ternary((N, *dims, co), 0.5, co + dims[2] + 1, device=DEV)
    X.assert_exact_cap(N * dims[0] * dims[1] * dims[2], 1.0, what=name)
    want = _conv_wgrad_ref(dy, a, k, (1, 1, 1), tuple(v // 2 for v in k))
    dW = ops.conv3d_wgrad(a, dy, k)
    _same(dW, want, name)
    with _Knobs(conv_wgrad_mfma=0):
        dW0 = ops.conv3d_wgrad(a, dy, k)
    assert torch.equal(dW0, dW)
    assert torch.equal(ops.conv3d_wgrad(a, dy, k), dW)


STRIDED_CASES = [("monai_c5_down1_32to64", 1, (24, 256, 256), 32, 64),
                 ("monai_c5_down2_64to128", 1, (12, 128, 128), 64, 128),
                 ("rsunet_like_down_N2_24to40", 2, (18, 160, 160), 24, 40)]


@pytest.mark.parametrize("name,N,big,ck,co", STRIDED_CASES, ids=[c[0] for c in STRIDED_CASES])
def test_conv3d_wgrad_strided_exact(name, N, big, ck, co):
    """k 3 / stride 2 / pad 1 weight gradient (the strided conv; with the operands swapped, the transposed conv's)."""
    nat, ops = _ops()
    small = tuple((v + 1) // 2 for v in big)
    ws = nat.lib().pytc_conv3d_wgrad_strided_ws_elems(N, ops._i3(small), ck, co, ops._i3((3, 3, 3)))
    # the workspace query bounds the slot counts of both plans (VALU / matrix core): a bound, not the launch's count
    print(f"[{name}] workspace bound {ws // (27 * ck * co)} slots")
    assert ws // (27 * ck * co) > 1
    b = X.ternary((N, *big, ck), 0.5, ck + big[1], device=DEV)
    s = X.ternary((N, *small, co), 0.5, co + small[1], device=DEV)
    X.assert_exact_cap(N * small[0] * small[1] * small[2], 1.0, what=name)
    want = _conv_wgrad_ref(s, b, (3, 3, 3), (2, 2, 2), (1, 1, 1))
    dW = ops.conv3d_wgrad_strided(b, s, (3, 3, 3), (2, 2, 2), (1, 1, 1))
    _same(dW, want, name)
    assert torch.equal(ops.conv3d_wgrad_strided(b, s, (3, 3, 3), (2, 2, 2), (1, 1, 1)), dW)


# ------------------------------------------------------------------------------------------------ UpCat / UNETR up-sampling deconvs
def _fold_replicate(d_up, lo_dims):
    """gradient of replicate-padding a (2 lo)-grid to the skip's grid: an extra last plane folds into the plane before it"""
    for ax in range(3):
        n2 = 2 * lo_dims[ax]
        if d_up.shape[1 + ax] == n2 + 1:
            last = d_up.narrow(1 + ax, n2, 1)
            d_up = d_up.narrow(1 + ax, 0, n2).clone()
            d_up.narrow(1 + ax, n2 - 1, 1).add_(last)
    return d_up


# (name, N, low dims, C_in, C_u, C_e, skip dims): BasicUNet's probe (filters 32..512, 2 x 64x128x128) and tutorial (8 / 16, 32x64x64)
UPCAT_CASES = [("probe_u1_64to64_e32", 2, (32, 64, 64), 64, 64, 32, (64, 128, 128)),
               ("probe_u2_128to64_e64", 2, (16, 32, 32), 128, 64, 64, (32, 64, 64)),
               ("probe_u4_512to256_e256", 2, (4, 8, 8), 512, 256, 256, (8, 16, 16)),
               ("probe_u1_odd_skip", 2, (32, 64, 63), 64, 64, 32, (65, 128, 127)),
               ("tutorial_u1_16to16_e8", 1, (16, 32, 32), 16, 16, 8, (32, 64, 64)),
               ("tutorial_u2_odd_skip", 1, (8, 16, 16), 16, 8, 16, (17, 33, 32))]


def _upcat_id(c):
    name, N, lo, ci, cu, ce, sk = c
    return f"{name}-splits{X.upcat_wgrad_splits(N * lo[0] * lo[1] * lo[2], ci, cu)}"


@pytest.mark.parametrize("c", UPCAT_CASES, ids=_upcat_id)
def test_upcat_deconv2_wgrad_exact(c):
    nat, ops = _ops()
    name, N, lo, ci, cu, ce, sk = c
    rows = N * lo[0] * lo[1] * lo[2]
    splits = X.upcat_wgrad_splits(rows, ci, cu)
    assert nat.lib().pytc_upcat_deconv2_wgrad_ws_elems(rows, ci, cu, nat.BF16) == splits * (ci + 1) * 8 * cu and splits > 1
    x_low = X.ternary((N, *lo, ci), 0.5, ci + lo[2], device=DEV)
    dcat = X.ternary((N, *sk, ce + cu), 0.5, cu + sk[2], device=DEV)
    weight = torch.zeros((ci, cu, 2, 2, 2), dtype=torch.float32, device=DEV)
    d_up = _fold_replicate(dcat[..., ce:].double(), lo)
    X.assert_exact_cap(2 * rows * 8 * 2, 1.0, what=name)                     # a folded plane doubles a term at most, per axis
    want = _conv_wgrad_ref(x_low, d_up, (2, 2, 2), (2, 2, 2), (0, 0, 0))   # (C_in, C_u, 2, 2, 2)
    want_b = dcat[..., ce:].double().reshape(-1, cu).sum(0)
    _, _, dW, db = ops.upcat_deconv2_bwd(dcat, x_low, weight, ce, want_dx_e=False, want_dx_low=False)
    _same(dW, want, "dW")
    _same(db, want_b, "db")
    _, _, dW2, db2 = ops.upcat_deconv2_bwd(dcat, x_low, weight, ce, want_dx_e=False, want_dx_low=False)
    assert torch.equal(dW2, dW) and torch.equal(db2, db)


# UNETR decoder deconvs (k 2, s 2, up channels first): default UNETR (hidden 768, feature_size 16) at 96^3 / 16 = 6^3 tokens, batch 2
DECONV_CASES = [("unetr_dec5_768to256_e256", 2, (6, 6, 6), 768, 256, 256),
                ("unetr_dec2_64to32_e32", 2, (24, 24, 24), 64, 32, 32),
                ("unetr_dec1_32to16_e16", 2, (48, 48, 48), 32, 16, 16),
                ("unetr_prup_768to128", 2, (6, 6, 6), 768, 128, 0)]


@pytest.mark.parametrize("c", DECONV_CASES,
                         ids=[f"{c[0]}-splits{X.upcat_wgrad_splits(c[1] * c[2][0] * c[2][1] * c[2][2], c[3], c[4])}" for c in DECONV_CASES])
def test_deconv2_upfirst_wgrad_exact(c):
    nat, ops = _ops()
    name, N, lo, ci, cu, ce = c
    rows = N * lo[0] * lo[1] * lo[2]
    splits = X.upcat_wgrad_splits(rows, ci, cu)
    assert nat.lib().pytc_upcat_deconv2_wgrad_ws_elems(rows, ci, cu, nat.BF16) == splits * (ci + 1) * 8 * cu and splits > 1
    x_low = X.ternary((N, *lo, ci), 0.5, ci + lo[0], device=DEV)
    dout = X.ternary((N, *(2 * v for v in lo), cu + ce), 0.5, cu + lo[0], device=DEV)
    weight = torch.zeros((ci, cu, 2, 2, 2), dtype=torch.float32, device=DEV)
    X.assert_exact_cap(rows, 1.0, what=name)
    want = _conv_wgrad_ref(x_low, dout[..., :cu], (2, 2, 2), (2, 2, 2), (0, 0, 0))
    _, _, dW, db = ops.deconv2_upfirst_bwd(dout, x_low, weight, ce, want_dx_e=False, want_dx_low=False, want_b=True)
    _same(dW, want, "dW")
    _same(db, dout[..., :cu].double().reshape(-1, cu).sum(0), "db")
    _, _, dW2, _ = ops.deconv2_upfirst_bwd(dout, x_low, weight, ce, want_dx_e=False, want_dx_low=False)
    assert torch.equal(dW2, dW)


# ------------------------------------------------------------------------------------------------ UNETR token linears
# (name, tokens M, K, N, dtype): the probe's default UNETR (batch 8 of 216 / 512 tokens, hidden 768) takes the MFMA route, the tutorial's
# 192-wide model (qkv 192 -> 576) and fp32 take the FMA route (one thread per output sums all rows in order: no slots).  The MLP GEMMs
# (768 x 3072) fill the machine with channel tiles and never split rows: the attention projections are the split cases
LINEAR_CASES = [("probe_b8_proj_768to768", 8 * 216, 768, 768, torch.bfloat16),
                ("probe128_b8_qkv_768to2304", 8 * 512, 768, 2304, torch.bfloat16),
                ("tutorial_qkv_192to576_fma", 2 * 64, 192, 576, torch.bfloat16),
                ("probe_b2_qkv_768to2304_fp32_fma", 2 * 216, 768, 2304, torch.float32)]


def _lin_id(c):
    name, M, K, N, dt = c
    mfma = dt == torch.bfloat16 and K % 64 == 0 and N % 128 == 0
    return f"{name}-" + (f"mfma-slots{X.pw_launch_slots(M, K, N)}" if mfma else "fma-inorder")


@pytest.mark.parametrize("c", LINEAR_CASES, ids=_lin_id)
def test_linear_wgrad_exact(c):
    nat, ops = _ops()
    name, M, K, N, dt = c
    x = X.ternary((M, K), 0.5, M + K, dtype=dt, device=DEV)
    dy = X.ternary((M, N), 0.5, M + N, dtype=dt, device=DEV)
    w = torch.zeros((N, K), dtype=torch.float32, device=DEV)
    mfma = ops.linear_mfma_applies(dy, K, N)
    assert mfma == ("mfma" in _lin_id(c))
    X.assert_exact_cap(M, 1.0, what=name)
    want = dy.double().t() @ x.double()
    if mfma:                                             # the route is pw_wgrad(N = 1): the library's own slot count of that launch
        dr = ops.DeferredReduce()
        ops.pw_wgrad(x, dy, N=1, rows_per_sample=M, c_in=K, c_out=N, defer=dr)
        assert dr.items[0][3] == X.pw_launch_slots(M, K, N) > 1
        dr.flush()
    _, dW, db, _ = ops.linear_bwd(dy, x, w, want_dx=False, want_w=True, want_b=True)
    _same(dW, want, "dW")
    _same(db, dy.double().sum(0), "db")
    _, dW2, db2, _ = ops.linear_bwd(dy, x, w, want_dx=False, want_w=True, want_b=True)
    assert torch.equal(dW2, dW) and torch.equal(db2, db)


# ------------------------------------------------------------------------------------------------ LayerNorm parameter gradients
def _ln_operands(rows, C, seed, last_rows, dt=torch.bfloat16):
    """x rows with a nonzero mean and spread (small integers), dy ternary: sparse (1 in 64 rows) except dense on the last slot's rows
    (last_rows: boolean (rows,) mask)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.randint(-3, 5, (rows, C), generator=g, device=DEV).float()).to(dt)
    dens = torch.where(last_rows, 1.0, 1.0 / 64)
    dy = X.ternary((rows, C), 1.0, seed + 1, dtype=dt, device=DEV, row_density=dens)
    return x, dy


def _contiguous_last(rows, slots):
    m = torch.zeros(rows, dtype=torch.bool)
    m[X.slot_rows(rows, slots)[-1][0]:] = True
    return m


def _ln_ref(x, dy, eps):
    xd = x.double()
    mu = xd.mean(1, keepdim=True)
    var = ((xd - mu) ** 2).mean(1, keepdim=True)
    xh = (xd - mu) / torch.sqrt(var + eps)
    return dy.double() * xh


def _check_ln(name, dg, db, x, dy, eps, rows_per_slot, slots, last_rows):
    t = _ln_ref(x, dy, eps)
    _same(db, dy.double().sum(0), f"{name} dbeta")
    abs_sum = t.abs().sum(0)
    bound = X.slot_rounding_bound(rows_per_slot, slots, abs_sum)
    err = (dg.double() - t.sum(0)).abs()
    assert bool((err <= bound).all()), f"{name} dgamma: max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3g}"
    # the case can see a lost last slot: its rows move some dgamma by more than twice the bound
    last = t[last_rows.to(t.device)].sum(0).abs()
    assert bool((last > 2 * bound).any()), f"{name}: dropping the last slot stays inside the bound; reshape the case"


# UNETR: default hidden 768 at batch 2 of 6^3 tokens (probe) and batch 8; SwinUNETR: stage 0 of the tutorial's 64^3 patch (32^3 tokens,
# C 48) and the 96 / 192-channel stages below it; MedNeXt channels-first LayerNorm at level 0
WIDE_CASES = [("unetr_probe_b2_768", 2 * 216, 768), ("unetr_probe_b8_768", 8 * 216, 768), ("unetr_tutorial_b2_192", 2 * 64, 192)]


@pytest.mark.parametrize("name,rows,C", WIDE_CASES, ids=[f"{n}-slots{X.layernorm_wide_slots(r)}" for n, r, _ in WIDE_CASES])
def test_layernorm_wide_param_grads(name, rows, C):
    nat, ops = _ops()
    slots = X.layernorm_wide_slots(rows)
    assert nat.lib().pytc_layernorm_wide_bwd_slots(rows) == slots > 1
    last = _contiguous_last(rows, slots)
    x, dy = _ln_operands(rows, C, rows + C, last)
    gamma = torch.ones(C, dtype=torch.float32, device=DEV)
    _, dg, db = ops.layernorm_wide_bwd(dy, x, gamma, 1e-5)
    _check_ln(name, dg, db, x, dy, 1e-5, 32, slots, last)
    _, dg2, db2 = ops.layernorm_wide_bwd(dy, x, gamma, 1e-5)
    assert torch.equal(dg2, dg) and torch.equal(db2, db)


ANY_CASES = [("swin_tutorial_stage0_32c_48", 32 ** 3, 48), ("swin_tutorial_stage1_16c_96", 2 * 16 ** 3, 96),
             ("swin_probe_stage0_48c_48", 48 ** 3, 48)]


@pytest.mark.parametrize("name,rows,C", ANY_CASES, ids=[f"{n}-slots{X.layernorm_any_slots(r)}" for n, r, _ in ANY_CASES])
def test_layernorm_any_param_grads(name, rows, C):
    nat, ops = _ops()
    slots = X.layernorm_any_slots(rows)
    assert nat.lib().pytc_layernorm_any_bwd_slots(rows) == slots > 1
    last = _contiguous_last(rows, slots)
    x, dy = _ln_operands(rows, C, rows + C, last)
    gamma = torch.ones(C, dtype=torch.float32, device=DEV)
    _, dg, db = ops.layernorm_any_bwd(dy, x, gamma, 1e-5)
    _check_ln(name, dg, db, x, dy, 1e-5, 256, slots, last)
    _, dg2, db2 = ops.layernorm_any_bwd(dy, x, gamma, 1e-5)
    assert torch.equal(dg2, dg) and torch.equal(db2, db)


# MedNeXt's LayerNorm variant (channels-first LayerNorm per voxel row): level 0 and level 3 of the 4 x 112^3 step (grid-stride blocks at
# the 1024-block cap) and level 2 (one pass)
ROWS_CASES = [("mednext_ln_L0_C32", 4 * 112 ** 3, 32), ("mednext_ln_L3_C256", 4 * 14 ** 3, 256), ("mednext_ln_L2_C128", 28 ** 3, 128)]


@pytest.mark.parametrize("name,rows,C", ROWS_CASES, ids=[f"{n}-slots{X.layernorm_rows_slots(r, c)}" for n, r, c in ROWS_CASES])
def test_layernorm_rows_param_grads(name, rows, C):
    """layernorm_rows_bwd returns (slots, 2, C) partials, which the training step reduces through DeferredReduce (training/autograd.py):
    the reduced sums are dbeta (exact) and dgamma (bound)."""
    nat, ops = _ops()
    slots = X.layernorm_rows_slots(rows, C)
    assert nat.lib().pytc_layernorm_rows_bwd_slots(rows, C, nat.BF16) == slots > 1
    rpb = X.layernorm_rows_rpb(C)
    last = (torch.arange(rows) // rpb) % slots == slots - 1            # rows of the last block (grid-stride over row blocks)
    x, dy = _ln_operands(rows, C, rows + C, last)
    gamma = torch.ones(C, dtype=torch.float32, device=DEV)
    _, part = ops.layernorm_rows_bwd(dy, x, gamma, 1e-5)
    assert tuple(part.shape) == (slots, 2, C)
    ssum = torch.empty((2, C), dtype=torch.float32, device=DEV)      # the training step's reduction of these partials
    dr = ops.DeferredReduce()
    dr.add(part, ssum, 2 * C, part.shape[0], keep=part)
    dr.flush()
    dg, db = ssum[1], ssum[0]
    _check_ln(name, dg, db, x, dy, 1e-5, -(-rows // slots), slots, last)
    _, part2 = ops.layernorm_rows_bwd(dy, x, gamma, 1e-5)
    assert torch.equal(part2, part)


# ------------------------------------------------------------------------------------------------ level-0 mixer backward (hp rebuilt)
def _sps_id(name, N, rows, sps):
    rps = -(-rows // sps)
    ragged = rows % rps != 0
    return f"{name}-slots{N * sps}" + ("-ragged" if ragged else "") + ("-mfma_block_at_sample_end" if rows % 32 else "")


def _mixer_id(c):
    name, N, rows, c_hid, div, gn = c
    return _sps_id(name + f"_div{div}" + ("_gn" if gn else ""), N, rows, X.mixer_bwd_rc_sps(N, rows, c_hid, slot_div=div))


# (name, N, rows per sample, C_hid, mixer_bwd_rc_slot_div, GroupNorm form): MedNeXt-S level 0 (C = C_out = 32, hidden 64) at 4 x 112^3,
# the odd batches and a ragged odd shape; the knob's two slot layouts; the GroupNorm form (per-sample slots + norm sums)
MIXER_CASES = [("L0_4x112", 4, 112 ** 3, 64, 1, False), ("L0_4x112", 4, 112 ** 3, 64, 2, False),
               ("L0_4x112", 4, 112 ** 3, 64, 1, True),
               ("odd_N3_32x48x64", 3, 32 * 48 * 64, 64, 1, False), ("odd_N5_16x80x48", 5, 16 * 80 * 48, 64, 1, True),
               ("odd_N3_33x47x61", 3, 33 * 47 * 61, 64, 1, False), ("odd_N3_33x47x61", 3, 33 * 47 * 61, 64, 1, True),
               ("odd_N3_33x47x61_hid96", 3, 33 * 47 * 61, 96, 1, False)]


def _mixer_operands(N, rows, C, c_hid, seed, same_affine):
    """t in {0, 1}; per-(sample, channel) affine a t + b in {(16, 0), (-16, 16)} -> {0, 16}; W2 one-hot (hp[h] = xn[h mod C]), b2 = 0:
    hp in {0, 16}, where gelu is exact and gelu_fast_with_grad's derivative is exactly 1 / 0.5; W3 ternary"""
    t = X.binary((N, rows, C), 0.5, seed, value=1.0, device=DEV)
    g = torch.Generator().manual_seed(seed + 1)
    neg = torch.rand(N, C, generator=g) < 0.5
    if same_affine:                                                 # GroupNorm form: a = gamma rstd must hold for every sample
        neg = neg[:1].expand(N, C)
    ab = torch.stack([torch.where(neg, -16.0, 16.0), torch.where(neg, 16.0, 0.0)], 1).contiguous().to(DEV)
    w2 = torch.zeros((c_hid, C), dtype=torch.float32, device=DEV)
    w2[torch.arange(c_hid), torch.arange(c_hid) % C] = 1.0
    w3 = X.ternary((32, c_hid), 0.5, seed + 2, dtype=torch.float32, device=DEV)
    dy = X.ternary((N, rows, 32), 0.5, seed + 3, device=DEV)
    xn = t.double() * ab[:, 0].double()[:, None] + ab[:, 1].double()[:, None]
    hp = xn[..., torch.arange(c_hid, device=DEV) % C]
    return t, ab, w2, w3, dy, xn, hp


@pytest.mark.parametrize("c", MIXER_CASES, ids=_mixer_id)
def test_mixer_bwd_rc_exact(c):
    """dW3 / db3 of the level-0 mixer backward (pytc_mixer_bwd_rc, hp rebuilt from t) in both slot layouts of mixer_bwd_rc_slot_div; in
    the GroupNorm form also dW2 / db2 and the per-sample norm sums s = (sum dtn, sum dtn xhat) with mean 0, rstd 1 (xhat = t exactly)."""
    nat, ops = _ops()
    name, N, rows, c_hid, div, gn = c
    C = 32
    assert ops.mixer_bwd_rc_supported(C, c_hid, 32, torch.bfloat16) >= (2 if gn else 1)
    t, ab, w2, w3, dy, xn, hp = _mixer_operands(N, rows, C, c_hid, rows + c_hid, same_affine=gn)
    dyd = dy.double().reshape(-1, 32)
    X.assert_exact_cap(X.gemm_abs_bound(16.0, dyd.abs().sum(0)), 16.0, what=name)
    want3 = dyd.t() @ hp.reshape(-1, c_hid)
    kw = dict(N=N, rows_per_sample=rows, c=C, c_hid=c_hid, c_out=32)
    extra = {}
    if gn:
        gamma = ab[0, 0].clone()                                    # a = gamma * rstd, b = beta - mean rstd gamma with mean 0, rstd 1
        assert torch.equal(ab[:, 0], gamma.expand(N, C))            # (the affine must then be the same for every sample)
        mr = torch.stack([torch.zeros(N, C), torch.ones(N, C)], 1).contiguous().to(DEV)
        extra = dict(mean_rstd=mr, w2=w2, gamma=gamma, count=float(rows))
    with _Knobs(mixer_bwd_rc_slot_div=div):
        sps = nat.lib().pytc_mixer_bwd_rc_sps(N, rows, c_hid)
        assert sps == X.mixer_bwd_rc_sps(N, rows, c_hid, slot_div=div) and N * sps > 1
        dr = ops.DeferredReduce()
        out = ops.mixer_bwd_rc(t, ab, dy, ops.packed_paired(w2), torch.zeros(c_hid, device=DEV), ops.packed_paired(w3, transposed=True),
                               defer=dr, **kw, **extra)
        assert dr.items[0][3] == N * sps
        dr.flush()
        out2 = ops.mixer_bwd_rc(t, ab, dy, ops.packed_paired(w2), torch.zeros(c_hid, device=DEV), ops.packed_paired(w3, transposed=True),
                                **kw, **extra)
    dW3, db3, dhp = out[:3]
    _same(dW3, want3, "dW3")
    _same(db3, dyd.sum(0), "db3")
    for a_, b_ in zip(out, out2):
        assert torch.equal(a_, b_)                                  # run to run (and deferred == own reduction)
    # dhp = (W3^T dy) gelu'(hp), gelu'(0) = 1/2, gelu'(16) = 1: small dyadics, exact in bf16
    dhp_want = (dyd @ w3.double()).view(N, rows, c_hid) * torch.where(hp == 16, 1.0, 0.5)
    _same(dhp.float(), dhp_want, "dhp")
    if gn:
        dW2, db2, s, _coef = out[3:]
        dh = dhp_want.reshape(-1, c_hid)
        _same(dW2, dh.t() @ xn.reshape(-1, C), "dW2")
        _same(db2, dh.sum(0), "db2")
        dtn = dhp_want @ w2.double()                                # gradient of the norm output
        _same(s[:, 0], dtn.sum(1), "s: sum dtn")
        _same(s[:, 1], (dtn * t.double()).sum(1), "s: sum dtn xhat")


# ------------------------------------------------------------------------------------------------ GroupNorm-fed expand conv
GN_CASES = [("L0_4x112_32to64", 4, 112 ** 3, 32, 64), ("L1_4x56_64to128", 4, 56 ** 3, 64, 128), ("L3_4x14_256to512", 4, 14 ** 3, 256, 512),
            ("odd_N3_33x47x61_32to64", 3, 33 * 47 * 61, 32, 64), ("odd_N5_16x80x48_32to64", 5, 16 * 80 * 48, 32, 64)]


@pytest.mark.parametrize("c", GN_CASES, ids=lambda c: _sps_id(c[0], c[1], c[2], X.pw_wgrad_groupnorm_sps(c[1], c[2], c[3], c[4])))
def test_pw_wgrad_groupnorm_exact(c):
    """pytc_pw_wgrad_groupnorm (per-sample slots, xhat operand split into bf16 high / low parts) with exact statistics: mean in {-1, 0, 1},
    rstd in {1/2, 1, 2} per (sample, channel), gamma in {+-1, +-2}, beta in {-1, 0, 1}: xhat, the affine and every sum are exact, so dW2,
    db2 and the norm sums s equal fp64."""
    nat, ops = _ops()
    name, N, rows, C, c_hid = c
    sps = nat.lib().pytc_pw_wgrad_groupnorm_sps(N, rows, C, c_hid)
    assert sps == X.pw_wgrad_groupnorm_sps(N, rows, C, c_hid) and N * sps > 1
    seed = rows + C
    t = X.ternary((N, rows, C), 0.5, seed, device=DEV)
    g = torch.Generator().manual_seed(seed + 1)
    mean = torch.randint(-1, 2, (N, C), generator=g).float()
    rstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (N, C), generator=g)]
    gamma = torch.tensor([1.0, -1.0, 2.0, -2.0])[torch.randint(0, 4, (C,), generator=g)]
    beta = torch.randint(-1, 2, (C,), generator=g).float()
    a = gamma * rstd
    ab = torch.stack([a, beta - mean * a], 1).contiguous().to(DEV)
    mr = torch.stack([mean, rstd], 1).contiguous().to(DEV)
    dhp = X.ternary((N, rows, c_hid), 1.0 / 16, seed + 2, device=DEV)       # |xn| <= 9: sparse enough for the cap at 4 x 112^3
    w2 = X.ternary((c_hid, C), 0.5, seed + 3, dtype=torch.float32, device=DEV)
    xhat = (t.double() - mr[:, 0].double()[:, None]) * mr[:, 1].double()[:, None]
    xn = xhat * gamma.double().to(DEV) + beta.double().to(DEV)
    dh = dhp.double()
    X.assert_exact_cap(X.gemm_abs_bound(float(xn.abs().max()), dh.reshape(-1, c_hid).abs().sum(0)), 0.5, what=name)
    dr = ops.DeferredReduce()
    dW2, db2, s, _coef = ops.pw_wgrad_groupnorm(t, mr, ab, dhp, w2, gamma.to(DEV), N=N, rows_per_sample=rows, c=C, c_hid=c_hid,
                                                count=float(rows), defer=dr)
    dr.flush()
    _same(dW2, dh.reshape(-1, c_hid).t() @ xn.reshape(-1, C), "dW2")
    _same(db2, dh.reshape(-1, c_hid).sum(0), "db2")
    dtn = dh @ w2.double()
    _same(s[:, 0], dtn.sum(1), "s: sum dtn")
    _same(s[:, 1], (dtn * xhat).sum(1), "s: sum dtn xhat")
    dW2b, db2b, sb, _ = ops.pw_wgrad_groupnorm(t, mr, ab, dhp, w2, gamma.to(DEV), N=N, rows_per_sample=rows, c=C, c_hid=c_hid,
                                               count=float(rows))
    assert torch.equal(dW2b, dW2) and torch.equal(db2b, db2) and torch.equal(sb, s)


# ------------------------------------------------------------------------------------------------ depthwise conv / stem statistics
def _stats_check(st, y64, name):
    """slot partials (N, slots, 2, C) of (sum y, sum y^2): their slot-order fp32 sum equals fp64 over all rows, every slot of every sample
    holds a nonzero sum y^2 (so losing or doubling any slot changes the total), under the fp32 cap"""
    N, slots, _, C = st.shape
    assert slots > 1
    yy = y64.reshape(N, -1, C)
    X.assert_exact_cap(float((yy * yy).sum(1).max()), 1.0, what=name)
    tot = X.slot_order_sum(st.transpose(0, 1))                   # (N, 2, C)
    _same(tot[:, 0], yy.sum(1), f"{name} sum y")
    _same(tot[:, 1], (yy * yy).sum(1), f"{name} sum y^2")
    assert bool((st[:, :, 1].sum(-1) > 0).all()), f"{name}: a slot without signal"


def _dwconv_ref(x, taps, bias=None):
    """fp64 stride-1 3x3x3 depthwise correlation of channels-last x (zero padding) with taps (27, C) [kz, ky, kx order]"""
    N, D, H, W, C = x.shape
    xp = F.pad(x.double(), (0, 0, 1, 1, 1, 1, 1, 1))
    y = torch.zeros((N, D, H, W, C), dtype=torch.float64, device=x.device)
    for i in range(27):
        kz, ky, kx = i // 9, (i // 3) % 3, i % 3
        y += xp[:, kz:kz + D, ky:ky + H, kx:kx + W] * taps[i].double()
    if bias is not None:
        y += bias.double()
    return y


DWSTAT_CASES = [("L0_4x112_C32", 4, (112, 112, 112), 32), ("L1_4x56_C64", 4, (56, 56, 56), 64), ("L3_4x14_C256", 4, (14, 14, 14), 256),
                ("odd_N3_33x47x61_C32", 3, (33, 47, 61), 32)]


@pytest.mark.parametrize("c", DWSTAT_CASES, ids=lambda c: c[0])
def test_dwconv3d_stat_slots_exact(c):
    """the forward depthwise conv's statistic slots (bf16 stride 1: z-march / matrix-core forms, fp16 nine-tap partials): sparse ternary
    x and taps keep every nine-tap partial below 2^11 and every statistic below 2^24"""
    nat, ops = _ops()
    name, N, dims, C = c
    x = X.ternary((N, *dims, C), 1.0 / 16, C + dims[0], device=DEV)
    taps = X.ternary((27, C), 0.5, C + 1, dtype=torch.float32, device=DEV)
    X.assert_exact_cap(9 * 1.0, 1.0, cap=X.EXACT_F16, what=name)       # |nine-tap partial| <= 9 max|x| max|w|
    slots = nat.lib().pytc_dwconv3d_stat_slots(N, *dims, C, 3, 1, nat.BF16, 0)
    print(f"[{name}] stat slots {slots}")
    y, st = ops.dwconv3d(x, taps, None, K=3, stride=1)
    assert st.shape[1] == slots > 1
    y64 = _dwconv_ref(x, taps)
    _same(y.float(), y64, f"{name} y")
    _stats_check(st, y64, name)
    assert torch.equal(ops.dwconv3d(x, taps, None, K=3, stride=1)[1], st)


STEM_CASES = [("L0_4x112", 4, (112, 112, 112)), ("odd_N3_33x47x60", 3, (33, 47, 60))]      # (the stem kernel takes W % 4 == 0)


@pytest.mark.parametrize("c", STEM_CASES, ids=lambda c: c[0])
def test_stem_dwconv3d_stat_slots_exact(c):
    """the fused stem (1 -> 32 pointwise) + depthwise conv with its statistic slots: ternary input, stem weights in {+-1}, stem bias
    in {-1, 0, 1} on a quarter of the channels, sparse ternary taps, integer bias"""
    nat, ops = _ops()
    name, N, dims = c
    C = 32
    assert ops.stem_dwconv3d_supported(1, C, 3)
    seed = dims[0] + N
    x = X.ternary((N, *dims, 1), 1.0 / 8, seed, dtype=torch.float32, device=DEV)
    g = torch.Generator().manual_seed(seed)
    sw = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0).to(DEV)
    sb = (torch.randint(-1, 2, (C,), generator=g) * (torch.arange(C) % 4 == 0)).float().to(DEV)
    taps = X.ternary((27, C), 1.0 / 8, seed + 1, dtype=torch.float32, device=DEV)
    bias = torch.randint(-2, 3, (C,), generator=g).float().to(DEV)
    X.assert_exact_cap(9 * 2.0, 1.0, cap=X.EXACT_F16, what=name)       # nine-tap partial of |stem(x)| <= 2
    s = x.double() * sw.double() + sb.double()                       # stem output (N, D, H, W, C), zero padded by the conv
    y64 = _dwconv_ref(s, taps, bias)
    assert float(y64.abs().max()) <= 256                              # exact in bf16
    slots = nat.lib().pytc_stem_dwconv3d_stat_slots(*dims)
    print(f"[{name}] stat slots {slots}")
    y, st = ops.stem_dwconv3d(x, ops.stem_dwconv3d_pack(sw, sb, taps, bias))
    assert st.shape[1] == slots > 1
    _same(y.float(), y64, f"{name} y")
    _stats_check(st, y64, name)

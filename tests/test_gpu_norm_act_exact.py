"""The norm / activation / pool kernel chain of the dense-conv models (RSUNet, MONAI U-Net, BasicUNet, the UNETR and SwinUNETR decoders)
against fp64, through the library's entry points (tests/norm_act_exact_cases.py holds the operands, references and derivations).

Exact operands make the correct result the fp64 result bit for bit: affine_act, act_bwd, the fused act_norm_bwd_stats / _apply pair at
slot counts above one, with idle row lanes, a ragged last slot, N > 1 and a second channel window, norm_bwd_means with padded channel
groups, and max pooling with ties and floor remainders are held to zero difference.  The finalize kernels (rsqrt, divisions) and the
BatchNorm running buffers are held to the bounds derived in the case module, ELU / sigmoid / tanh to the margins measured in
profiles/norm_act_exact_probe.txt."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import norm_act_exact_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ops():
    from pytorch_connectomics_amd import _native as nat, hip_ops as ops
    return nat, ops


class _ScalarForm:
    """the scalar elementwise kernels for a block (ops.set_tuning("elementwise_vec", 0)), the default restored afterwards"""

    def __enter__(self):
        _ops()[1].set_tuning("elementwise_vec", 0)

    def __exit__(self, *exc):
        _ops()[1].set_tuning("elementwise_vec", 1)
        return False


def _same(got: torch.Tensor, want64: torch.Tensor, what: str, rounded: bool = False) -> None:
    """zero difference with the fp64 reference.  rounded: the result carries its one rounding to the storage type (dx in bf16), so it
    is compared with the storage image of the reference; otherwise the reference itself must be representable"""
    assert tuple(got.shape) == tuple(want64.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(want64.shape)}"
    d = (got.double() - want64.to(got.dtype).double()).abs()
    lost = (want64.to(got.dtype).double() - want64).abs()
    assert rounded or float(lost.max()) == 0.0, f"{what}: the reference is not representable in {got.dtype}: not an exact case"
    assert float(d.max()) == 0.0, f"{what}: {int((d != 0).sum())} of {d.numel()} off, max |diff| {float(d.max())} (exact inputs: must be 0)"


def _same_bits(got: torch.Tensor, want64: torch.Tensor, what: str) -> None:
    _same(got, want64, what)
    ne = K.bits(got) != K.bits(want64.to(got.dtype))
    assert not bool(ne.any()), f"{what}: {int(ne.sum())} values differ in the sign of a zero"


def _within(got: torch.Tensor, want64: torch.Tensor, bound: torch.Tensor, what: str) -> None:
    d = (got.double() - want64).abs()
    over = d > bound
    ratio = float((d / bound.clamp_min(1e-300)).max())
    print(f"{what}: max |diff| {float(d.max()):.3e}, largest diff / bound {ratio:.3f}")
    assert not bool(over.any()), f"{what}: {int(over.sum())} of {d.numel()} over the derived bound, worst diff / bound {ratio:.3f}"


# ------------------------------------------------------------------------------------------------ 1, 2: elementwise forward / backward
_EW_IDS = [f"{s}-{'x'.join(map(str, sh))}" for s, sh in K.ELEMENTWISE_SHAPES]


@pytest.mark.parametrize("with_ab", [True, False], ids=["ab", "noab"])
@pytest.mark.parametrize("storage,shape", K.ELEMENTWISE_SHAPES, ids=_EW_IDS)
def test_affine_act_is_exact_in_both_forms(storage, shape, with_ab):
    nat, ops = _ops()
    x, _, ab = K.elementwise_operands(storage, shape, seed=shape[-1] + shape[0], with_ab=with_ab, device=DEV)
    for name, act, prm, _ in K.EXACT_ACTS[:3]:
        want = K.ref_affine_act(x, ab, act, prm)
        with _ScalarForm():
            ys = ops.affine_act(x, ab, act, prm)
        _same(ys, want, f"affine_act scalar {name}")
        yv = ops.affine_act(x, ab, act, prm)
        _same(yv, want, f"affine_act {name}")
        if K.has_vec(shape[-1], x.dtype):
            assert torch.equal(K.bits(yv), K.bits(ys)), f"affine_act {name}: vector and scalar forms differ"


@pytest.mark.parametrize("with_ab", [True, False], ids=["ab", "noab"])
@pytest.mark.parametrize("storage,shape", K.ELEMENTWISE_SHAPES, ids=_EW_IDS)
def test_act_bwd_is_exact_in_both_forms(storage, shape, with_ab):
    nat, ops = _ops()
    x, da, ab = K.elementwise_operands(storage, shape, seed=shape[-1] + shape[0], with_ab=with_ab, device=DEV)
    assert bool(((K.ref_t(x, ab, x.dtype) == 0) & torch.signbit(K.ref_t(x, ab, x.dtype))).any()), "no t == -0.0 voxel in the case"
    for name, act, prm, prelu in K.EXACT_ACTS:
        wt, wp = K.ref_act_bwd(da, x, ab, act, prm)
        with _ScalarForm():
            dts, dps = ops.act_bwd(da, x, ab, act, prm, want_prelu=prelu)
        dtv, dpv = ops.act_bwd(da, x, ab, act, prm, want_prelu=prelu)
        for form, dt, dp in (("scalar", dts, dps), ("default", dtv, dpv)):
            _same_bits(dt, wt, f"act_bwd {form} {name} dt")
            assert (dp is not None) == prelu
            if prelu:
                _same_bits(dp, wp, f"act_bwd {form} {name} dp")


_SMOOTH = [("elu", K.ACT_ELU, 1.0), ("sigmoid", K.ACT_SIGMOID, 0.0), ("tanh", K.ACT_TANH, 0.0)]


@pytest.mark.parametrize("with_ab", [True, False], ids=["ab", "noab"])
@pytest.mark.parametrize("storage,C", [("bf16", 24), ("bf16", 5), ("f32", 20), ("f32", 5)])
def test_smooth_activations_stay_within_the_measured_margin(storage, C, with_ab):
    """ELU / sigmoid / tanh forward and the ELU derivative: bound = K.smooth_bound (profiles/norm_act_exact_probe.txt)"""
    nat, ops = _ops()
    shape = (2, 3, 5, 7, C)
    x, da, ab = K.smooth_operands(storage, shape, seed=C, with_ab=with_ab, device=DEV)
    t = K.ref_t(x, ab)
    for form in ("scalar", "default"):
        for name, act, prm in _SMOOTH:
            want = K.act64(t, act, prm)
            if form == "scalar":
                with _ScalarForm():
                    y = ops.affine_act(x, ab, act, prm)
            else:
                y = ops.affine_act(x, ab, act, prm)
            _within(y, want, K.smooth_bound(name, want, storage, t=t, ab=with_ab), f"affine_act {form} {name} {storage}")
        tb = K.ref_t(x, ab, x.dtype)
        want = da.double() * K.act_der64(tb, K.ACT_ELU, 1.0)
        if form == "scalar":
            with _ScalarForm():
                dt, _ = ops.act_bwd(da, x, ab, K.ACT_ELU, 1.0)
        else:
            dt, _ = ops.act_bwd(da, x, ab, K.ACT_ELU, 1.0)
        bound = da.double().abs() * (K.INTRINSIC_MARGIN["elu_der"] + K.U32) + (2.0 ** -8 if storage == "bf16" else K.U32) * want.abs()
        _within(dt, want, bound, f"act_bwd {form} elu {storage}")


# ------------------------------------------------------------------------------------------------ 3: past the 16384-block grid cap
def test_affine_act_and_act_bwd_past_the_grid_cap_vector_form():
    nat, ops = _ops()
    shape = K.GRID_CAP_VEC_SHAPE
    n = 1
    for v in shape:
        n *= v
    assert n // 8 > K.GRID_CAP
    x, da, ab = K.elementwise_operands("bf16", shape, seed=3, with_ab=True, device=DEV)
    y = ops.affine_act(x, ab, K.ACT_LEAKY, K.SLOPE)
    _same(y, K.ref_affine_act(x, ab, K.ACT_LEAKY, K.SLOPE), "affine_act past the grid cap")
    del y
    dt, dp = ops.act_bwd(da, x, ab, K.ACT_LEAKY, K.SLOPE, want_prelu=True)
    wt, wp = K.ref_act_bwd(da, x, ab, K.ACT_LEAKY, K.SLOPE)
    _same_bits(dt, wt, "act_bwd dt past the grid cap")
    _same_bits(dp, wp, "act_bwd dp past the grid cap")


def test_affine_act_and_act_bwd_past_the_grid_cap_scalar_form():
    nat, ops = _ops()
    shape = K.GRID_CAP_SCALAR_SHAPE
    n = 1
    for v in shape:
        n *= v
    assert n > K.GRID_CAP and shape[-1] % 8
    x, da, ab = K.elementwise_operands("bf16", shape, seed=4, with_ab=True, device=DEV)
    _same(ops.affine_act(x, ab, K.ACT_LEAKY, K.SLOPE), K.ref_affine_act(x, ab, K.ACT_LEAKY, K.SLOPE), "affine_act scalar past the grid cap")
    dt, dp = ops.act_bwd(da, x, ab, K.ACT_LEAKY, K.SLOPE, want_prelu=True)
    wt, wp = K.ref_act_bwd(da, x, ab, K.ACT_LEAKY, K.SLOPE)
    _same_bits(dt, wt, "act_bwd scalar dt past the grid cap")
    _same_bits(dp, wp, "act_bwd scalar dp past the grid cap")


# ------------------------------------------------------------------------------------------------ 4, 5, 10: the fused backward pair
_FUSED = K.FUSED_CASES + [K.WINDOW_CASE]


def _fused_setup(c, with_ab=True):
    o = K.fused_operands(c, seed=c.rows + c.C, with_ab=with_ab, device=DEV)
    for what, q in K.fused_caps(c, o).items():
        assert q < K.EXACT_F32, f"{c.name} {what}: {q:.3g} quanta"
    return o


def _slot_partials(c, o, act, prm, prelu):
    """the per-slot partials of pytc_act_norm_bwd_stats in a workspace of this test's own, pre-filled with NaN"""
    nat, ops = _ops()
    n_ws = nat.lib().pytc_norm_bwd_ws_elems(c.N, c.rows, c.C)
    ws = torch.full((n_ws + n_ws // 2,), float("nan"), dtype=torch.float32, device=DEV)
    s = torch.empty((c.N, 2, c.C), dtype=torch.float32, device=DEV)
    p = torch.empty((c.N, c.C), dtype=torch.float32, device=DEV) if prelu else None
    ops._run("act_norm_bwd_stats", 0, nat.lib().pytc_act_norm_bwd_stats, ops._p(o["da"]), ops._p(o["x"]), ops._p(o["ab"]), ops._p(o["mr"]),
             ops._p(ws), ops._p(s), ops._p(ws[n_ws:]) if prelu else None, ops._p(p), c.N, c.rows, c.C, int(act), float(prm),
             ops.dtype_code(o["x"].dtype), ops._stream())
    torch.cuda.synchronize()
    return ws[:n_ws], ws[n_ws:], s, p


@pytest.mark.parametrize("c", _FUSED, ids=lambda c: c.name)
def test_act_norm_bwd_stats_slots_are_the_mirrors_row_ranges(c):
    """ops has no slot query for the fused pair: the slot count of the mirror is checked through the partials themselves, which must
    be the fp64 sums over the mirror's row ranges, with the rest of the workspace untouched"""
    slots = c.slots
    assert slots > 1
    o = _fused_setup(c)
    ws, pws, s, p = _slot_partials(c, o, K.ACT_LEAKY, K.SLOPE, True)
    used = c.N * slots * 2 * c.C
    assert bool(torch.isnan(ws[used:]).all()) and not bool(torch.isnan(ws[:used]).any()), "the launch did not write `slots` slots"
    assert bool(torch.isnan(pws[used // 2:]).all()) and not bool(torch.isnan(pws[:used // 2]).any())
    part, ppart = ws[:used].view(c.N, slots, 2, c.C), pws[:used // 2].view(c.N, slots, c.C)
    ranges = K.slot_rows(c.rows, slots)
    assert len(ranges) == slots and ranges[-1][1] == c.rows
    for i, r in enumerate(ranges):
        ws_, wp_ = K.ref_bwd_stats(o["da"], o["x"], o["ab"], o["mr"], K.ACT_LEAKY, K.SLOPE, rows=r)
        _same(part[:, i], ws_, f"{c.name} slot {i} rows {r}")
        _same(ppart[:, i], wp_, f"{c.name} slot {i} rows {r} (PReLU column)")
    assert float(part[:, -1].abs().max()) > 0, "the last slot must carry signal"


@pytest.mark.parametrize("with_ab", [True, False], ids=["ab", "noab"])
@pytest.mark.parametrize("c", _FUSED, ids=lambda c: c.name)
def test_act_norm_bwd_stats_is_exact(c, with_ab):
    nat, ops = _ops()
    assert c.slots > 1
    o = _fused_setup(c, with_ab)
    x, da, ab, mr = o["x"], o["da"], o["ab"], o["mr"]
    for name, act, prm, prelu in K.EXACT_ACTS:
        ws_, wp_ = K.ref_bwd_stats(da, x, ab, mr, act, prm)
        s, p = ops.act_norm_bwd_stats(da, x, ab, mr, act, prm, want_prelu=prelu)
        _same(s, ws_, f"{c.name} {name} s")
        assert (p is not None) == prelu
        if prelu:
            _same(p, wp_, f"{c.name} {name} p")
        # the three-pass route on the same operands
        dt, dp = ops.act_bwd(da, x, ab, act, prm, want_prelu=prelu)
        assert torch.equal(ops.norm_bwd_stats(dt, x, mr), s), f"{c.name} {name}: fused and three-pass statistics differ"
        if prelu:
            _same(p, ops.channel_stats(dp)[:, :, 0].double().sum(1), f"{c.name} {name} p against channel_stats(dp)")
        s2, p2 = ops.act_norm_bwd_stats(da, x, ab, mr, act, prm, want_prelu=prelu)
        assert torch.equal(s2, s) and (p is None or torch.equal(p2, p)), f"{c.name} {name}: a second run differs"


@pytest.mark.parametrize("c", _FUSED, ids=lambda c: c.name)
def test_act_norm_bwd_apply_is_exact(c):
    nat, ops = _ops()
    assert c.slots > 1
    o = _fused_setup(c)
    x, da, ab, mr, M = o["x"], o["da"], o["ab"], o["mr"], o["M"]
    gammas = [("full", o["gamma"]), ("none", None)]
    if c.gamma_short:
        gammas.append(("short", o["gamma"][:c.gamma_short].clone()))
    for name, act, prm, _ in K.EXACT_ACTS[:3]:
        dt, _ = ops.act_bwd(da, x, ab, act, prm)
        for gname, g in gammas:
            want = K.ref_bwd_apply(da, x, ab, mr, g, M, act, prm)
            dx = ops.act_norm_bwd_apply(da, x, ab, mr, g, M, act, prm)
            _same(dx, want, f"{c.name} {name} gamma {gname} dx", rounded=True)
            gz = K.zero_extended(g, c.C)
            gz = gz.contiguous() if gz is not None else None
            assert torch.equal(ops.norm_bwd_apply_general(dt, x, mr, gz, M), dx), f"{c.name} {name} {gname}: three-pass dx differs"
            with _ScalarForm():
                assert torch.equal(ops.norm_bwd_apply_general(dt, x, mr, gz, M), dx), f"{c.name} {name} {gname}: scalar three-pass dx"
    dx2 = ops.act_norm_bwd_apply(da, x, None, mr, None, M, K.ACT_RELU, 0.0)
    _same(dx2, K.ref_bwd_apply(da, x, None, mr, None, M, K.ACT_RELU, 0.0), f"{c.name} relu without affine dx", rounded=True)


def test_fused_backward_pair_refuses_unaligned_channels():
    """conditions PYTC_REQUIRE catches on the host: C not a multiple of 16 bytes, gamma longer than C"""
    nat, ops = _ops()
    x = torch.zeros(1, 64, 12, dtype=torch.bfloat16, device=DEV)
    mr = torch.zeros(1, 2, 12, device=DEV)
    with pytest.raises(RuntimeError):
        ops.act_norm_bwd_stats(x, x, None, mr, K.ACT_RELU, 0.0)
    with pytest.raises(RuntimeError):
        ops.act_norm_bwd_apply(x, x, None, mr, None, mr, K.ACT_RELU, 0.0)
    x = torch.zeros(1, 64, 16, dtype=torch.bfloat16, device=DEV)
    mr = torch.zeros(1, 2, 16, device=DEV)
    with pytest.raises(RuntimeError):
        ops.act_norm_bwd_apply(x, x, None, mr, torch.ones(17, device=DEV), mr, K.ACT_RELU, 0.0)


# ------------------------------------------------------------------------------------------------ 6: norm_bwd_means
@pytest.mark.parametrize("use_gamma", [True, False], ids=["gamma", "nogamma"])
@pytest.mark.parametrize("c", K.GROUP_CASES, ids=lambda c: c.name)
def test_norm_bwd_means_group_algebra(c, use_gamma):
    nat, ops = _ops()
    s, gamma = K.means_operands(c, seed=c.C + c.groups)
    g = gamma if use_gamma else None
    rows = K.MEANS_ROWS
    wM, wdg, wdb, bound = K.ref_means(s, g, c, rows)
    gd = g.to(DEV) if g is not None else None           # a tensor of its own with exactly groups * cpg entries
    M, dg, db = ops.norm_bwd_means(s.to(DEV), gd, c.groups, rows, want_gamma=True, want_beta=True, cpg=c.cpg)
    _same(dg.cpu(), wdg, f"{c.name} dgamma")
    _same(db.cpu(), wdb, f"{c.name} dbeta")
    assert float(M[:, :, c.c_real:].abs().max()) == 0.0 if c.c_real < c.C else True, f"{c.name}: M on the padded channels"
    if K.means_exact(c, rows):
        _same(M.cpu(), wM, f"{c.name} M")
    else:
        _within(M.cpu(), wM, bound, f"{c.name} M (two roundings)")
    Mn, dgn, dbn = ops.norm_bwd_means(s.to(DEV), gd, c.groups, rows, want_gamma=False, want_beta=False, cpg=c.cpg)
    assert dgn is None and dbn is None and torch.equal(Mn, M)
    if use_gamma:
        # nothing beyond gamma's groups * cpg entries is read: the same values followed by 1e30 give the same result
        longer = torch.full((c.c_real + 64,), 1e30, device=DEV)
        longer[:c.c_real] = gd
        M2, dg2, db2 = ops.norm_bwd_means(s.to(DEV), longer[:c.c_real], c.groups, rows, want_gamma=True, want_beta=True, cpg=c.cpg)
        assert torch.equal(M2, M) and torch.equal(dg2, dg) and torch.equal(db2, db), f"{c.name}: the result depends on what follows gamma"


def test_norm_bwd_means_refuses_groups_that_do_not_fit():
    nat, ops = _ops()
    s = torch.zeros(1, 2, 24, device=DEV)
    with pytest.raises(RuntimeError):
        ops.norm_bwd_means(s, None, 5, 64, want_gamma=False, want_beta=False, cpg=5)
    with pytest.raises(RuntimeError):
        ops.norm_bwd_means(s, None, 5, 64, want_gamma=False, want_beta=False)


# ------------------------------------------------------------------------------------------------ 7: norm_finalize_groups
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("slots", K.FINALIZE_SLOTS)
@pytest.mark.parametrize("c", [c for c in K.GROUP_CASES if c.groups], ids=lambda c: c.name)
def test_norm_finalize_groups_within_the_derived_bound(c, slots, affine):
    nat, ops = _ops()
    st = K.synthetic_stats(K.GROUP_N, slots, c.C, c.c_real, seed=slots + c.C)
    gamma, beta = K.general_gamma_beta(c.c_real, seed=c.C) if affine else (None, None)
    count = float(slots * K.STAT_ROWS_PER_SLOT)
    wab, wmr, bd, _ = K.ref_finalize(st, count, gamma, beta, 1e-5, c)
    gd, bdv = (gamma.to(DEV), beta.to(DEV)) if affine else (None, None)
    ab, mr = ops.norm_finalize_groups_mr(st.to(DEV), count, gd, bdv, 1e-5, c.groups, c.cpg)
    ab, mr = ab.cpu(), mr.cpu()
    tag = f"{c.name} slots {slots}"
    if c.c_real < c.C:
        for t in (ab, mr):
            assert float(t[:, :, c.c_real:].abs().max()) == 0.0, f"{tag}: padded channels must carry exactly 0"
    _within(ab[:, 0], wab[:, 0], bd["a"], f"{tag} a")
    _within(ab[:, 1], wab[:, 1], bd["b"], f"{tag} b")
    _within(mr[:, 0], wmr[:, 0], bd["mean"], f"{tag} mean")
    _within(mr[:, 1], wmr[:, 1], bd["rstd"], f"{tag} rstd")
    assert torch.equal(ops.norm_finalize_groups(st.to(DEV), count, gd, bdv, 1e-5, c.groups, c.cpg).cpu(), ab), f"{tag}: the form without mean / rstd"


def test_norm_finalize_groups_refuses_groups_that_do_not_fit():
    nat, ops = _ops()
    st = torch.zeros(1, 1, 2, 24, device=DEV)
    with pytest.raises(RuntimeError):
        ops.norm_finalize_groups_mr(st, 64.0, None, None, 1e-5, 5, 5)
    with pytest.raises(RuntimeError):
        ops.norm_finalize_groups_mr(st, 64.0, None, None, 1e-5, 5, 0)


# ------------------------------------------------------------------------------------------------ 8: BatchNorm finalize / running buffers
@pytest.mark.parametrize("momentum", K.BN_MOMENTA)
@pytest.mark.parametrize("slots_total", K.BN_SLOTS_TOTAL)
@pytest.mark.parametrize("c_real,C", K.BN_CASES)
def test_bn_train_finalize_and_running_buffers(c_real, C, slots_total, momentum):
    nat, ops = _ops()
    N = K.GROUP_N
    slots = slots_total // N
    st = K.synthetic_stats(N, slots, C, c_real, seed=slots_total + C)
    count = float(slots_total * K.STAT_ROWS_PER_SLOT)
    gamma, beta = K.general_gamma_beta(c_real, seed=C)
    rm0, rv0 = K.bn_old_running(c_real, seed=C + 1)
    forms = [("affine+running", gamma, beta, True), ("affine", gamma, beta, False), ("running", None, None, True)]
    if c_real == C:
        forms.append(("plain", None, None, False))
    for fname, g, b, running in forms:
        tag = f"bn {c_real}/{C} slots {slots_total} momentum {momentum} {fname}"
        w = K.ref_bn(st, count, g, b, K.BN_EPS, momentum, c_real, rm0 if running else None, rv0 if running else None)
        rm, rv = (rm0.clone().to(DEV), rv0.clone().to(DEV)) if running else (None, None)
        nbt = torch.tensor(41, dtype=torch.int64, device=DEV) if running else None
        ab, mr = ops.bn_train_finalize(st.to(DEV), count, g.to(DEV) if g is not None else None, b.to(DEV) if b is not None else None,
                                       K.BN_EPS, momentum, rm, rv, nbt, N)
        ab, mr = ab.cpu(), mr.cpu()
        assert tuple(ab.shape) == (N, 2, C) and tuple(mr.shape) == (N, 2, C)
        for n in range(1, N):
            assert torch.equal(ab[n], ab[0]) and torch.equal(mr[n], mr[0]), f"{tag}: sample {n} differs from sample 0"
        if c_real < C:
            assert float(ab[:, :, c_real:].abs().max()) == 0.0 and float(mr[:, :, c_real:].abs().max()) == 0.0, f"{tag}: tail"
        bd = w["bounds"]
        _within(ab[0, 0], w["a"], bd["a"], f"{tag} a")
        _within(ab[0, 1], w["b"], bd["b"], f"{tag} b")
        _within(mr[0, 0], w["mean"], bd["mean"], f"{tag} mean")
        _within(mr[0, 1], w["rstd"], bd["rstd"], f"{tag} rstd")
        if running:
            assert int(nbt) == 42, f"{tag}: num_batches_tracked {int(nbt)}"
            assert rm.numel() == c_real and rv.numel() == c_real
            _within(rm.cpu(), w["rmean"], w["rmean_bound"], f"{tag} running_mean")
            _within(rv.cpu(), w["rvar"], w["rvar_bound"], f"{tag} running_var")
            if momentum == 0.0:
                assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0), f"{tag}: momentum 0 must keep the buffers"
            # nn.BatchNorm3d itself in fp64 on data with these statistics is the blend ref_bn restates: checked on the CPU
            # (test_host_norm_act_exact_cases.py) against the module


@pytest.mark.parametrize("k", [1, 7])
@pytest.mark.parametrize("c_real", [18, 36, 16])
def test_bn_update_running_cumulative_average(c_real, k):
    """the momentum=None route: momentum 1 / k with exact (mean, rstd) inputs: the variance recovered from rstd has e_r = 0"""
    nat, ops = _ops()
    mr = K.exact_mean_rstd(1, c_real, seed=c_real + k)
    rm0, rv0 = K.bn_old_running(c_real, seed=c_real)
    count, mom = 3.0 * 9 * 16 * 20, 1.0 / k
    rm, rv = rm0.clone().to(DEV), rv0.clone().to(DEV)
    ops.bn_update_running(mr.to(DEV), rm, rv, count, K.BN_EPS, mom)
    mean, rstd = mr[0, 0].double(), mr[0, 1].double()
    var = 1.0 / (rstd * rstd) - K.BN_EPS
    w = K.ref_running(mean, var, 0.0, torch.zeros_like(mean), count, K.BN_EPS, mom, rm0, rv0)
    assert rm.numel() == c_real and rv.numel() == c_real
    _within(rm.cpu(), w["rmean"], w["rmean_bound"], f"bn_update_running C {c_real} k {k} running_mean")
    _within(rv.cpu(), w["rvar"], w["rvar_bound"], f"bn_update_running C {c_real} k {k} running_var")


# ------------------------------------------------------------------------------------------------ 9: the chain, smooth activation
@pytest.mark.parametrize("storage", ["bf16", "f32"])
@pytest.mark.parametrize("kind,c_real,groups", K.CHAIN_CASES, ids=[f"{k}{c}" for k, c, _ in K.CHAIN_CASES])
def test_norm_elu_chain_on_padded_channels(kind, c_real, groups, storage):
    """RA._norm_act forward and backward against fp64 autograd of norm -> ELU on the real channels.  Per tensor the rel-L2 limit is the
    larger of 2 x the fp32 CPU restatement's (K.CHAIN_RESTATED_REL_L2) and the measured ELU margins carried through the formulas:
    out: margin per element; dx = rstd P(gamma dt) with P an orthogonal projection, so |d dx|_2 <= max |rstd gamma| margin |da|_2;
    dgamma / dbeta: margin sum |da xhat| / sum |da| per channel"""
    from pytorch_connectomics_amd.models.architectures.rsunet import NormAct
    from pytorch_connectomics_amd.training.rsunet_autograd import _norm_act
    x, da, gamma, beta = K.chain_operands(kind, c_real, storage, seed=c_real + len(kind))
    C = x.shape[-1]
    na = NormAct(c_real, kind, "elu", num_groups=max(groups, 1), alpha=1.0).train()
    if gamma is not None:
        with torch.no_grad():
            na.norm.weight.copy_(gamma)
            na.norm.bias.copy_(beta)
    na = na.to(DEV)
    xc = x.to(DEV).requires_grad_()
    out = _norm_act(na, xc)
    out.backward(da.to(DEV))
    w = K.chain_ref(x, da, gamma, beta, kind, groups, c_real)
    o, dx = out.detach().cpu(), xc.grad.cpu()
    assert o.dtype == x.dtype and tuple(o.shape) == tuple(x.shape) and tuple(dx.shape) == tuple(x.shape)
    if C > c_real:
        assert float(o[..., c_real:].abs().max()) == 0.0 and float(dx[..., c_real:].abs().max()) == 0.0, "padded tail must stay 0"
    lim = {k: 2 * v for k, v in K.CHAIN_RESTATED_REL_L2[storage].items()}
    dan = float(da.double().norm())
    gmax = float(gamma.abs().max()) if gamma is not None else 1.0
    # every statistics group's variance is at least the smallest per-(sample, channel) variance (mean of them + variance of means)
    xr = x[..., :c_real].double().reshape(x.shape[0], -1, c_real)
    rstd_max = float(1.0 / xr.std(1, unbiased=False).min())
    xhat_max = 2.0 * float(xr.abs().max()) * rstd_max
    prop = {"out": K.INTRINSIC_MARGIN["elu"] * (w["out"].numel() ** 0.5) / float(w["out"].norm()),
            "dx": rstd_max * gmax * K.INTRINSIC_MARGIN["elu_der"] * dan / float(w["dx"].norm())}
    got = {"out": o[..., :c_real], "dx": dx[..., :c_real]}
    if gamma is not None:
        assert na.norm.weight.grad.numel() == c_real and na.norm.bias.grad.numel() == c_real
        got["dgamma"], got["dbeta"] = na.norm.weight.grad.cpu(), na.norm.bias.grad.cpu()
        for k, f in (("dgamma", xhat_max), ("dbeta", 1.0)):
            prop[k] = K.INTRINSIC_MARGIN["elu_der"] * f * float(da.double().abs().reshape(-1, C).sum(0).norm()) / float(w[k].norm())
    for k, v in got.items():
        r = K.rel_l2(v, w[k])
        limit = max(lim[k], prop[k])
        print(f"chain {kind}{c_real} {storage} {k}: rel-L2 {r:.3e} (limit {limit:.3e})")
        assert r <= limit, f"chain {kind}{c_real} {storage} {k}: rel-L2 {r:.3e} over {limit:.3e}"


# ------------------------------------------------------------------------------------------------ 11: max pooling
@pytest.mark.parametrize("factor", K.POOL_FACTORS, ids=lambda f: "x".join(map(str, f)))
@pytest.mark.parametrize("shape", K.POOL_SHAPES, ids=lambda s: f"C{s[-1]}")
@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_maxpool_with_ties_and_remainders_equals_torch(storage, shape, factor):
    nat, ops = _ops()
    dt = K.DTYPES[storage]
    x = K.pool_input(shape, seed=shape[-1], dtype=dt)
    dy = K.pool_grad(shape, factor, seed=shape[-1], dtype=dt)
    wy, wdx = K.ref_pool(x, dy, factor)
    y = ops.maxpool3d(x.to(DEV), factor).cpu()
    assert torch.equal(y, wy), f"maxpool3d {factor}: {int((y != wy).sum())} outputs differ from F.max_pool3d"
    dx = ops.maxpool3d_bwd(x.to(DEV), dy.to(DEV), factor).cpu()
    assert torch.equal(dx, wdx), f"maxpool3d_bwd {factor}: {int((dx != wdx).sum())} voxels differ from autograd (first maximum in z, y, x order)"
    rim = K.rim_mask(shape, factor)
    assert float(dx[:, rim].abs().max()) == 0.0 if bool(rim.any()) else True, "the floor-dropped rim of dx must be 0"


def test_every_pool_axis_leaves_a_remainder_for_some_factor():
    D, H, W = K.POOL_SHAPES[0][1:4]
    for ax, n in enumerate((D, H, W)):
        assert any(n % f[ax] for f in K.POOL_FACTORS), f"axis {ax}"


def test_maxpool_of_an_all_minus_inf_window_is_minus_inf():
    nat, ops = _ops()
    x = K.pool_input((1, 4, 4, 4, 5), seed=9, dtype=torch.float32)
    x[0, :2, :2, :2, 1] = float("-inf")
    x[0, 2:, 2:, 2:, 3] = float("-inf")
    x[0, 0, 0, 0, 0] = float("-inf")                       # a window with one -inf among finite values
    want, _ = K.ref_pool(x, None, (2, 2, 2))
    assert bool(torch.isinf(want).any())
    y = ops.maxpool3d(x.to(DEV), (2, 2, 2)).cpu()
    assert torch.equal(y, want), f"maxpool3d: all -inf windows give {y[torch.isinf(want)].tolist()}, torch gives -inf"

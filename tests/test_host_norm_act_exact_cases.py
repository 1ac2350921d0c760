"""CPU checks of the norm / activation / pool cases (tests/norm_act_exact_cases.py): the exactness premises hold for every table
entry, the slot mirrors give the counts the GPU cases assert, a plain fp32 restatement of each kernel formula passes every assertion
the GPU test makes (zero difference for the exact ones, the derived bound for the others), and restatements with one seeded defect each
fail them (the bounded ones by at least twice the bound)."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import exact_reduction_cases as X  # noqa: E402
import norm_act_exact_cases as K  # noqa: E402


def _eq(got, want64, rounded=False):
    """the GPU test's zero-difference assertion as a predicate"""
    w = want64.to(got.dtype)
    if not rounded and float((w.double() - want64).abs().max()) != 0.0:
        return False
    return float((got.double() - w.double()).abs().max()) == 0.0


def _eq_bits(got, want64):
    return _eq(got, want64) and bool((K.bits(got) == K.bits(want64.to(got.dtype))).all())


def _ratio(got, want64, bound):
    return float(((got.double() - want64).abs() / bound.clamp_min(1e-300)).max())


_ALL_FUSED = K.FUSED_CASES + [K.WINDOW_CASE]


# ------------------------------------------------------------------------------------------------ 1: exactness premises
@pytest.mark.parametrize("c", _ALL_FUSED, ids=lambda c: c.name)
def test_fused_case_premises(c):
    o = K.fused_operands(c, seed=c.rows + c.C)
    for what, q in K.fused_caps(c, o).items():
        assert q < K.EXACT_F32, f"{c.name} {what}: {q:.3g} quanta"
    x, da, ab, mr = o["x"], o["da"], o["ab"], o["mr"]
    assert set(x.float().abs().unique().tolist()) == {0.0, 1.0} and set(da.float().abs().unique().tolist()) == {0.0, 0.5}
    assert bool(torch.signbit(x.float())[x == 0].any()) and bool((~torch.signbit(x.float()))[x == 0].any())       # both zeros
    t = K.ref_t(x, ab)
    assert torch.equal(t.to(c.dtype).double(), t), "t = a x + b must survive the storage rounding"
    assert bool(((t == 0) & torch.signbit(t)).any()) and bool(((t == 0) & ~torch.signbit(t)).any()), "t == -0.0 and t == 0.0 voxels"
    for name, act, prm, _ in K.EXACT_ACTS:
        dt, dp = K.ref_act_bwd(da, x, ab, act, prm)
        for v in (dt, dp, K.act64(t, act, prm)):
            assert torch.equal(v.to(c.dtype).double(), v), f"{name}: not representable in {c.storage}"
    xh = K.ref_xhat(x, mr)
    assert torch.equal(xh.float().double(), xh)
    dx = K.ref_bwd_apply(da, x, ab, mr, o["gamma"], o["M"], K.ACT_LEAKY, K.SLOPE)
    assert torch.equal(dx.float().double(), dx), "dx before its single rounding must be exact in fp32"
    assert float(dx.abs().max()) * 2 ** 10 < K.EXACT_F32 and torch.equal((dx * 2 ** 10).round(), dx * 2 ** 10)     # few-bit dyadics
    # the last slot carries signal in every column
    last = X.slot_rows(c.rows, c.slots)[-1]
    s, p = K.ref_bwd_stats(da, x, ab, mr, K.ACT_LEAKY, K.SLOPE, rows=last)
    assert float(s[:, 0].abs().max()) > 0 and float(s[:, 1].abs().max()) > 0 and float(p.abs().max()) > 0


@pytest.mark.parametrize("storage,shape", K.ELEMENTWISE_SHAPES, ids=lambda v: str(v))
def test_elementwise_case_premises(storage, shape):
    x, da, ab = K.elementwise_operands(storage, shape, seed=shape[-1] + shape[0], with_ab=True)
    t = K.ref_t(x, ab)
    assert torch.equal(t.to(x.dtype).double(), t)
    assert bool(((t == 0) & torch.signbit(t)).any()) and bool(((t == 0) & ~torch.signbit(t)).any())
    if shape[0] > 1:
        assert not torch.equal(ab[0], ab[1]), "per-sample affines must differ"
    tn = K.ref_t(x, None)
    assert bool(((tn == 0) & torch.signbit(tn)).any())


def test_grid_cap_shapes_pass_the_cap_by_little():
    n = 1
    for v in K.GRID_CAP_VEC_SHAPE:
        n *= v
    assert K.GRID_CAP < n // 8 < 1.01 * K.GRID_CAP and K.GRID_CAP_VEC_SHAPE[-1] % 8 == 0
    n = 1
    for v in K.GRID_CAP_SCALAR_SHAPE:
        n *= v
    assert K.GRID_CAP < n < 1.01 * K.GRID_CAP and K.GRID_CAP_SCALAR_SHAPE[-1] % 8 != 0


@pytest.mark.parametrize("c", K.GROUP_CASES, ids=lambda c: c.name)
def test_group_case_premises(c):
    s, gamma = K.means_operands(c, seed=c.C + c.groups)
    assert gamma.numel() == c.c_real <= c.C
    assert float(s.abs().max()) * 4 * 2 * 9 * K.GROUP_N < K.EXACT_F32 and torch.equal((s * 4).round(), s * 4)
    if c.groups:
        for slots in K.FINALIZE_SLOTS:
            st = K.synthetic_stats(K.GROUP_N, slots, c.C, c.c_real, seed=slots + c.C)
            assert torch.equal(st, st.round()) and float(st.abs().sum(1).max()) * 9 < K.EXACT_F32
            assert float(st[..., c.c_real:].abs().max()) == 0.0 if c.c_real < c.C else True
            _, _, _, prem = K.ref_finalize(st, float(slots * K.STAT_ROWS_PER_SLOT), None, None, 1e-5, c)
            assert float(prem["mean"].abs().max()) <= 1.0 and 0.25 <= float(prem["var"].min()) and float(prem["var"].max()) <= 4.0
    assert {K.means_exact(c) for c in K.GROUP_CASES} == {True, False}
    assert all(K.means_exact(c) for c in K.GROUP_CASES if c.groups and c.width in (1, 2, 4, 8))
    assert {c.width for c in K.GROUP_CASES if c.groups and K.means_exact(c)} == {1, 2, 4, 8}


def test_the_unrolled_finalize_loop_and_its_tail_are_reached():
    """slots * cpg > 2048: eight slot rows in flight per thread; 400 x 6 = 2400 is one unrolled round plus a tail"""
    assert 400 in K.FINALIZE_SLOTS and any(c.width == 6 for c in K.GROUP_CASES)
    total = 400 * 6
    assert 0 + 7 * 256 < total and 255 + 7 * 256 < total          # every thread runs one unrolled round
    assert 2048 + 255 < total <= 2048 + 7 * 256                     # ... then the tail loop, and no second unrolled round
    assert any(s * c.width <= 2048 for s in K.FINALIZE_SLOTS for c in K.GROUP_CASES if c.groups)     # the plain loop alone
    assert 1024 * 9 > 4 * 2048                                      # several unrolled rounds


# ------------------------------------------------------------------------------------------------ 2: slot mirrors
def test_slot_mirrors_give_the_counts_the_gpu_cases_assert():
    assert [c.slots for c in K.FUSED_CASES] == [2, 2, 3, 2, 2, 2]
    assert K.WINDOW_CASE.slots == 2 and K.WINDOW_CASE.C // 8 == 257
    # one-slot controls: the shapes the earlier suite used (C = 16 on at most 990 rows, C = 12 is not served)
    assert K.act_norm_slots(990, 16, torch.bfloat16) == 1 and K.act_norm_slots(990, 16, torch.float32) == 1
    assert K.act_norm_slots(120, 12, torch.float32) == 1
    for c in _ALL_FUSED:
        assert c.slots <= X.colstats_slots(c.rows), "the workspace is sized for colstats_slots"
        sl = X.slot_rows(c.rows, c.slots)
        assert len(sl) == c.slots
    ragged = [c for c in K.FUSED_CASES if len({b - a for a, b in X.slot_rows(c.rows, c.slots)}) > 1]
    assert len(ragged) >= 4
    assert any(c.N > 1 and c in ragged for c in K.FUSED_CASES)
    idle = {(c.storage, c.C): K.row_lanes(c.C, c.dtype)[2] for c in K.FUSED_CASES}
    assert idle[("bf16", 24)] > 0 and idle[("bf16", 40)] > 0 and idle[("f32", 20)] > 0 and idle[("f32", 36)] > 0
    assert K.row_lanes(8, torch.bfloat16)[:2] == (1, 256)


def test_slot_mirror_matches_the_workspace_query():
    from pytorch_connectomics_amd import _native as nat
    if not nat.LIB_PATH.exists():
        pytest.skip(f"HIP library {nat.LIB_PATH} not built")
    for c in _ALL_FUSED:
        assert nat.lib().pytc_norm_bwd_ws_elems(c.N, c.rows, c.C) == c.N * X.colstats_slots(c.rows) * 2 * c.C


# ------------------------------------------------------------------------------------------------ 3, 4: restatements and defects
@pytest.mark.parametrize("storage,shape", K.ELEMENTWISE_SHAPES, ids=lambda v: str(v))
def test_elementwise_restatements_pass_and_defects_fail(storage, shape):
    x, da, ab = K.elementwise_operands(storage, shape, seed=shape[-1] + shape[0], with_ab=True)
    x3, da3 = x.reshape(shape[0], -1, shape[-1]), da.reshape(shape[0], -1, shape[-1])
    vecs = [1] + ([K.epv(x.dtype)] if K.has_vec(shape[-1], x.dtype) else [])
    for abv in (ab, None):
        for name, act, prm, prelu in K.EXACT_ACTS:
            wt, wp = K.ref_act_bwd(da3, x3, abv, act, prm)
            for vec in vecs:
                assert _eq(K.restate_affine_act(x3, abv, act, prm, vec=vec), K.ref_affine_act(x3, abv, act, prm))
                dt, dp = K.restate_act_bwd(da3, x3, abv, act, prm, vec=vec)
                assert _eq_bits(dt, wt) and _eq_bits(dp, wp)
            if act != K.ACT_NONE:
                assert not _eq_bits(K.restate_act_bwd(da3, x3, abv, act, prm, defect="kink_ge")[0], wt), f"{name}: kink at t >= 0 unseen"
            dpd = K.restate_act_bwd(da3, x3, abv, act, prm, defect="dp_le")[1]
            assert _eq(dpd, wp) and not _eq_bits(dpd, wp), "dp from t <= 0 differs only in the sign of zeros: the bit comparison sees it"
    if len(vecs) > 1:
        v = vecs[1]
        assert not _eq(K.restate_affine_act(x3, ab, K.ACT_LEAKY, K.SLOPE, vec=v, defect="sample_index"), K.ref_affine_act(x3, ab, K.ACT_LEAKY, K.SLOPE))
        assert not _eq_bits(K.restate_act_bwd(da3, x3, ab, K.ACT_LEAKY, K.SLOPE, vec=v, defect="sample_index")[0],
                            K.ref_act_bwd(da3, x3, ab, K.ACT_LEAKY, K.SLOPE)[0])


@pytest.mark.parametrize("c", _ALL_FUSED, ids=lambda c: c.name)
def test_fused_restatements_pass_and_defects_fail(c):
    o = K.fused_operands(c, seed=c.rows + c.C)
    x, da, ab, mr, M, gamma = o["x"], o["da"], o["ab"], o["mr"], o["M"], o["gamma"]
    act, prm = K.ACT_LEAKY, K.SLOPE
    ws, wp = K.ref_bwd_stats(da, x, ab, mr, act, prm)
    s, p = K.restate_bwd_stats(da, x, ab, mr, act, prm, c.slots)
    assert _eq(s, ws) and _eq(p, wp)
    s1, p1 = K.restate_bwd_stats(da, x, ab, mr, act, prm, 1)
    assert torch.equal(s1, s) and torch.equal(p1, p), "any slot count gives the same bits"
    defects = ["last_slot", "slot_off_by_one", "kink_ge"] + (["sample_index"] if c.N > 1 else [])
    for d in defects:
        sd, pd = K.restate_bwd_stats(da, x, ab, mr, act, prm, c.slots, defect=d)
        assert not _eq(sd, ws), f"{c.name}: defect {d} unseen in s"
        if d != "kink_ge":
            assert not _eq(pd, wp), f"{c.name}: defect {d} unseen in p"
    gammas = [gamma, None] + ([gamma[:c.gamma_short]] if c.gamma_short else [])
    for g in gammas:
        want = K.ref_bwd_apply(da, x, ab, mr, g, M, act, prm)
        assert _eq(K.restate_bwd_apply(da, x, ab, mr, g, M, act, prm, c.slots), want, rounded=True)
        for d in defects:
            assert not _eq(K.restate_bwd_apply(da, x, ab, mr, g, M, act, prm, c.slots, defect=d), want, rounded=True), f"{c.name}: {d} unseen in dx"
    if c.gamma_short:
        g = gamma[:c.gamma_short]
        want = K.ref_bwd_apply(da, x, ab, mr, g, M, act, prm)
        assert not _eq(K.restate_bwd_apply(da, x, ab, mr, g, M, act, prm, c.slots, defect="gamma_tail"), want, rounded=True)


@pytest.mark.parametrize("use_gamma", [True, False])
@pytest.mark.parametrize("c", K.GROUP_CASES, ids=lambda c: c.name)
def test_means_restatement_passes_and_defects_fail(c, use_gamma):
    s, gamma = K.means_operands(c, seed=c.C + c.groups)
    g = gamma if use_gamma else None
    wM, wdg, wdb, bound = K.ref_means(s, g, c, K.MEANS_ROWS)
    M, dg, db = K.restate_means(s, g, c, K.MEANS_ROWS)
    assert _eq(dg, wdg) and _eq(db, wdb)
    exact = K.means_exact(c)
    assert _eq(M, wM) if exact else _ratio(M, wM, bound) <= 1.0
    if c.c_real < c.C:
        assert float(M[:, :, c.c_real:].abs().max()) == 0.0
    if c.groups == 0:
        return
    defects = (["group_shift"] if c.groups > 1 or c.c_real < c.C else []) + (["pad_counted"] if c.C // c.groups != c.width else [])
    for d in defects:
        Md = K.restate_means(s, g, c, K.MEANS_ROWS, defect=d)[0]
        if exact:
            assert not _eq(Md, wM), f"{c.name}: {d} unseen"
        else:
            worst = float(((Md.double() - wM).abs() - 2 * bound).max())
            assert worst > 0 and _ratio(Md, wM, bound) >= 2.0, f"{c.name}: {d} within twice the bound"
        if c.c_real < c.C:
            assert float(Md[:, :, c.c_real:].abs().max()) > 0, f"{c.name}: {d} leaves the padded M at 0"


@pytest.mark.parametrize("slots", K.FINALIZE_SLOTS)
@pytest.mark.parametrize("c", [c for c in K.GROUP_CASES if c.groups], ids=lambda c: c.name)
def test_finalize_restatement_passes_and_defects_fail(c, slots):
    st = K.synthetic_stats(K.GROUP_N, slots, c.C, c.c_real, seed=slots + c.C)
    count = float(slots * K.STAT_ROWS_PER_SLOT)
    for gamma, beta in (K.general_gamma_beta(c.c_real, seed=c.C), (None, None)):
        wab, wmr, bd, _ = K.ref_finalize(st, count, gamma, beta, 1e-5, c)

        def worst(ab, mr):
            return max(_ratio(ab[:, 0], wab[:, 0], bd["a"]), _ratio(ab[:, 1], wab[:, 1], bd["b"]),
                       _ratio(mr[:, 0], wmr[:, 0], bd["mean"]), _ratio(mr[:, 1], wmr[:, 1], bd["rstd"]))

        ab, mr = K.restate_finalize(st, count, gamma, beta, 1e-5, c)
        assert worst(ab, mr) <= 1.0, f"{c.name} slots {slots}: the fp32 restatement is at {worst(ab, mr):.2f} of the bound"
        if c.c_real < c.C:
            assert float(ab[:, :, c.c_real:].abs().max()) == 0.0 and float(mr[:, :, c.c_real:].abs().max()) == 0.0
        defects = (["last_slot"] if slots > 1 else []) + (["group_shift"] if c.groups > 1 or c.c_real < c.C else []) + \
                  (["pad_counted"] if c.C // c.groups != c.width else [])
        for d in defects:
            abd, mrd = K.restate_finalize(st, count, gamma, beta, 1e-5, c, defect=d)
            tail = float(abd[:, :, c.c_real:].abs().max()) + float(mrd[:, :, c.c_real:].abs().max()) if c.c_real < c.C else 0.0
            assert worst(abd, mrd) >= 2.0 or tail > 0, f"{c.name} slots {slots}: {d} within twice the bound ({worst(abd, mrd):.2f})"


@pytest.mark.parametrize("momentum", K.BN_MOMENTA)
@pytest.mark.parametrize("slots_total", K.BN_SLOTS_TOTAL)
@pytest.mark.parametrize("c_real,C", K.BN_CASES)
def test_bn_restatement_passes_and_defects_fail(c_real, C, slots_total, momentum):
    N = K.GROUP_N
    st = K.synthetic_stats(N, slots_total // N, C, c_real, seed=slots_total + C)
    count = float(slots_total * K.STAT_ROWS_PER_SLOT)
    gamma, beta = K.general_gamma_beta(c_real, seed=C)
    rm0, rv0 = K.bn_old_running(c_real, seed=C + 1)
    w = K.ref_bn(st, count, gamma, beta, K.BN_EPS, momentum, c_real, rm0, rv0)
    assert float(w["premise"]["mean"].abs().max()) <= 1.0 and 0.25 <= float(w["premise"]["var"].min()) <= float(w["premise"]["var"].max()) <= 4.0
    bd = w["bounds"]

    def worst(r, running=True):
        a, b, mean, rstd, nm, nv = r
        v = max(_ratio(a, w["a"], bd["a"]), _ratio(b, w["b"], bd["b"]), _ratio(mean, w["mean"], bd["mean"]), _ratio(rstd, w["rstd"], bd["rstd"]))
        if running:
            v = max(v, _ratio(nm, w["rmean"], w["rmean_bound"]), _ratio(nv, w["rvar"], w["rvar_bound"]))
        return v

    r = K.restate_bn(st, count, gamma, beta, K.BN_EPS, momentum, c_real, rm0, rv0)
    assert worst(r) <= 1.0, f"restatement at {worst(r):.2f} of the bound"
    assert r[4].numel() == c_real and float(r[0][c_real:].abs().sum()) == 0.0
    if momentum == 0.0:
        assert torch.equal(r[4], rm0) and torch.equal(r[5], rv0)
    for d in ["last_slot"] + (["pad_counted"] if c_real < C else []):
        assert worst(K.restate_bn(st, count, gamma, beta, K.BN_EPS, momentum, c_real, rm0, rv0, defect=d), running=momentum > 0) >= 2.0, d


def test_ref_bn_is_batchnorm3d_in_fp64():
    """the blend ref_bn states is nn.BatchNorm3d's own: on data in fp64, from that data's sums"""
    torch.manual_seed(0)
    c_real, N = 18, 3
    x = torch.randn(N, c_real, 4, 5, 6, dtype=torch.float64) * 1.3 + 0.4
    bn = torch.nn.BatchNorm3d(c_real, eps=K.BN_EPS, momentum=0.1).double().train()
    rm0, rv0 = K.bn_old_running(c_real, seed=5)
    with torch.no_grad():
        bn.running_mean.copy_(rm0)
        bn.running_var.copy_(rv0)
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_()
    y = bn(x).detach()
    xc = x.permute(0, 2, 3, 4, 1).reshape(N, 1, -1, c_real)
    st = torch.stack([xc.sum(2), (xc * xc).sum(2)], 2)                       # (N, 1, 2, C) in fp64
    w = K.ref_bn(st, float(N * 120), bn.weight.detach(), bn.bias.detach(), K.BN_EPS, 0.1, c_real, rm0, rv0)
    assert float((w["rmean"] - bn.running_mean).abs().max()) < 1e-12 and float((w["rvar"] - bn.running_var).abs().max()) < 1e-12
    want = x * w["a"].view(1, -1, 1, 1, 1) + w["b"].view(1, -1, 1, 1, 1)
    assert float((want - y).abs().max()) < 1e-12
    assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("k", [1, 7])
def test_running_restatement_from_exact_rstd(k):
    c_real = 18
    mr = K.exact_mean_rstd(1, c_real, seed=c_real + k)
    rm0, rv0 = K.bn_old_running(c_real, seed=c_real)
    count, mom = 3.0 * 9 * 16 * 20, 1.0 / k
    mean, rstd = mr[0, 0], mr[0, 1]
    w = K.ref_running(mean.double(), 1.0 / (rstd.double() ** 2) - K.BN_EPS, 0.0, torch.zeros(c_real, dtype=torch.float64), count, K.BN_EPS, mom, rm0, rv0)
    nm, nv = K.restate_running(mean, rstd, count, K.BN_EPS, mom, rm0, rv0)
    assert _ratio(nm, w["rmean"], w["rmean_bound"]) <= 1.0 and _ratio(nv, w["rvar"], w["rvar_bound"]) <= 1.0
    # the biased variance in place of the unbiased one is seen
    nvb = (1.0 - torch.tensor(mom)) * rv0 + torch.tensor(mom) * (1.0 / (rstd * rstd) - K.BN_EPS)
    assert _ratio(nvb, w["rvar"], w["rvar_bound"]) >= 2.0


@pytest.mark.parametrize("factor", K.POOL_FACTORS, ids=lambda f: "x".join(map(str, f)))
@pytest.mark.parametrize("shape", K.POOL_SHAPES, ids=lambda s: f"C{s[-1]}")
@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_pool_restatement_passes_and_defects_fail(storage, shape, factor):
    dt = K.DTYPES[storage]
    x = K.pool_input(shape, seed=shape[-1], dtype=dt)
    dy = K.pool_grad(shape, factor, seed=shape[-1], dtype=dt)
    wy, wdx = K.ref_pool(x, dy, factor)
    y, dx = K.restate_pool(x, dy, factor)
    assert torch.equal(y, wy) and torch.equal(dx, wdx)
    rim = K.rim_mask(shape, factor)
    if bool(rim.any()):
        assert float(wdx[:, rim].abs().max()) == 0.0
        assert not torch.equal(K.restate_pool(x, dy, factor, defect="rim")[1], wdx), "an uncleared rim is unseen"
    if factor[0] * factor[1] * factor[2] > 1:
        assert not torch.equal(K.restate_pool(x, dy, factor, defect="tie_last")[1], wdx), "ties routed to the last maximum are unseen"
    assert float((wdx != 0).sum()) == dy.numel(), "every output gradient lands on exactly one voxel"


def test_every_pool_axis_leaves_a_remainder_for_some_factor():
    D, H, W = K.POOL_SHAPES[0][1:4]
    for ax, n in enumerate((D, H, W)):
        assert any(n % f[ax] for f in K.POOL_FACTORS), f"axis {ax}"


def test_pool_minus_inf_window_separates_the_two_starting_values():
    x = K.pool_input((1, 4, 4, 4, 5), seed=9, dtype=torch.float32)
    x[0, :2, :2, :2, 1] = float("-inf")
    want, _ = K.ref_pool(x, None, (2, 2, 2))
    assert torch.equal(K.restate_pool(x, None, (2, 2, 2))[0], want)
    assert not torch.equal(K.restate_pool(x, None, (2, 2, 2), init=-3.402823466e38)[0], want)
    xb = x.bfloat16()                                  # in bf16 the finite start rounds to -inf when stored: fp32 alone can differ
    assert torch.equal(K.restate_pool(xb, None, (2, 2, 2), init=-3.402823466e38)[0], K.ref_pool(xb, None, (2, 2, 2))[0])


# ------------------------------------------------------------------------------------------------ the chain
@pytest.mark.parametrize("storage", ["bf16", "f32"])
@pytest.mark.parametrize("kind,c_real,groups", K.CHAIN_CASES, ids=[f"{k}{c}" for k, c, _ in K.CHAIN_CASES])
def test_chain_restatement_passes_the_chain_assertion(kind, c_real, groups, storage):
    """the restatement's own rel-L2 depends a little on the CPU's summation order: it must pass what the GPU case asserts (twice the
    recorded value), not reproduce the record"""
    x, da, gamma, beta = K.chain_operands(kind, c_real, storage, seed=c_real + len(kind))
    C = x.shape[-1]
    assert C == K.pad_channels(c_real, x.dtype) and (C == c_real or float(x[..., c_real:].abs().max()) == 0.0)
    w = K.chain_ref(x, da, gamma, beta, kind, groups, c_real)
    r = K.chain_ref(x, da, gamma, beta, kind, groups, c_real, dtype=torch.float32, storage=x.dtype)
    for k, v in K.CHAIN_RESTATED_REL_L2[storage].items():
        if w[k] is not None:
            assert K.rel_l2(r[k], w[k]) <= 2 * v, f"{kind}{c_real} {storage} {k}: {K.rel_l2(r[k], w[k]):.4e} recorded {v:.4e}"


def test_the_mirrored_constants_are_the_librarys():
    from pytorch_connectomics_amd import _native as nat
    assert (K.ACT_NONE, K.ACT_SIGMOID, K.ACT_TANH, K.ACT_RELU, K.ACT_LEAKY, K.ACT_ELU) == \
        (nat.ACT_NONE, nat.ACT_SIGMOID, nat.ACT_TANH, nat.ACT_RELU, nat.ACT_LEAKY, nat.ACT_ELU)
    from pytorch_connectomics_amd import hip_ops as ops
    for c in (5, 18, 36, 24, 3):
        for dt in (torch.bfloat16, torch.float32):
            assert K.pad_channels(c, dt) == ops.pad_channels(c, dt)

"""CPU checks of the epilogue case module (tests/epilogue_exact_cases.py): the generators are seeded and produce only the stated value
sets, every exactness cap holds for every GPU case (the case table is shared: an over-cap case fails here), the fp64 references agree
with torch double-precision autograd of training/module.py's formulas, a dropped or doubled last slot changes the exact sums of every
multi-slot case, and the Python mirrors equal the library's host-side queries."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import epilogue_exact_cases as E  # noqa: E402
import exact_reduction_cases as X  # noqa: E402

CASES = E.loss_cases()


def test_the_case_table_covers_what_it_claims():
    by = {c.name: c for c in CASES}
    assert {c.R for c in CASES} >= {16383, 16384, 32767, 32768, 32769, 112 ** 3, 18 * 256 * 256, 24 * 256 * 256, 160 ** 3}
    assert [E.loss_slots(r) for r in (16383, 16384, 32767, 32768, 32769)] == [1, 1, 1, 2, 2]
    assert by["w112"].slots == 85 and by["w18x256"].slots == 72 and by["w24x256"].slots == 96 and by["w160"].slots == 250
    assert by["cap256"].R > 256 * 16384 and by["cap256"].slots == 256 and "ragged" in by["cap256"].id and "ragged" in by["w112"].id
    assert any(c.N * c.C > 1 for c in CASES) and any(c.N == 4 and c.C == 3 and c.R == 112 ** 3 for c in CASES)
    assert any(len(c.spatial) == 2 for c in CASES)
    assert {c.layout for c in CASES if c.R == 112 ** 3} == {"contig", "cl", "cl_slice", "crop"}
    assert {c.tdtype for c in CASES if c.R == 112 ** 3} == {"float", "uint8", "bool"}
    assert any(c.weight == "bcast" and c.R == 112 ** 3 for c in CASES)
    assert {c.pw for c in CASES} == {None, 0.5, 2.0}
    assert any(c.den_rounded for c in CASES) and any(c.snr == 1e-5 for c in CASES)
    # the backward: 4 passes of 1024-row blocks up to 2048 blocks, more beyond
    assert E.loss_bwd_passes(2097151) == 4 and E.loss_bwd_passes(2097153) == 5 and E.loss_bwd_passes(160 ** 3) == 8
    assert E.loss_bwd_blocks(5940) == 6 and E.loss_bwd_blocks(2097153) == 2048
    assert len({c.id for c in CASES}) == len(CASES)


def test_generators_are_seeded_and_produce_only_the_stated_values():
    c = next(k for k in CASES if k.name == "edge32769")
    x, t, w = E.loss_operands(c)
    x2, t2, w2 = E.loss_operands(c)
    assert torch.equal(x, x2) and torch.equal(t, t2) and (w is None or torch.equal(w, w2))
    assert not torch.equal(E.loss_operands(c, seed=1)[0], E.loss_operands(c, seed=2)[0])
    for k in CASES:
        if k.R > 40000:
            continue
        x, t, w = E.loss_operands(k)
        want = {-128.0, 128.0} | ({0.0} if k.family == 2 else set())
        assert set(x.unique().tolist()) == want and set(t.float().unique().tolist()) == {0.0, 1.0}
        assert t.dtype == {"float": torch.float32, "uint8": torch.uint8, "bool": torch.bool}[k.tdtype]
        if w is not None:
            assert set(w.unique().tolist()) <= set(k.wvals) and w.shape[1] == (1 if k.weight == "bcast" else k.C)
    assert set(E.ternary_grad((3, 5000), 0.5, 1, scale=0.25).unique().tolist()) == {-0.25, 0.0, 0.25}
    assert float(E.probe_grad(8193, "last").sum()) == 1.0 and float(E.probe_grad(8193, "chunk_ends").sum()) == 5.0   # chunk 2: one element
    assert float(E.probe_grad(8192, "chunk_ends").sum()) == 4.0
    b = E.blobs((2, 1, 24, 40, 36), 3)
    assert set(b.unique().tolist()) == {0.0, 1.0} and torch.equal(b, E.blobs((2, 1, 24, 40, 36), 3))
    from pytorch_connectomics_amd.training.cldice_autograd import _soft_erode_pool, soft_skeleton_torch
    e = b
    for _ in range(3):
        e = _soft_erode_pool(e)
    assert float(e.sum()) > 0, "the blobs survive three erosions: the later skeleton levels carry signal"
    assert set(soft_skeleton_torch(b, 5).unique().tolist()) == {0.0, 1.0}
    assert set(E.cldice_weight((2, 1, 8, 8, 8), 1).unique().tolist()) == {0.0, 0.5, 1.0, 2.0}
    x, t, w = E.clamp_range_operands("grid", (2, 2, 8, 10, 12), 5)
    assert float(x.min()) == -20.0 and float(x.max()) == 20.0 and 0 <= float(t.min()) and float(t.max()) <= 1
    assert float(w.min()) == 0.0 and float(w.max()) <= 2.0 and bool((w[:, :, :2] == 0).all())


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_loss_caps_hold_and_the_last_slot_carries_signal(c):
    """every cap of every GPU case on the drawn operands; dropping or doubling the last slot moves every exactly asserted sum of
    every (n, c) by a nonzero integer amount (all sums are exact in any order, so the slot-split emulation of a fault is the exact
    sum minus / plus the last slot's: test_slot_emulation_matches_the_shortcut holds that equivalence to slot_split_sum_f32)"""
    x, t, w = E.loss_operands(c)
    s = E.loss_assert_caps(c, x, t, w)
    assert E.loss_ws_elems(c.N, c.C, c.R) == c.slots * c.N * c.C * 5
    if c.slots == 1:
        return
    a, b = X.slot_rows(c.R, c.slots)[-1]
    tail = E.loss_sums64(x.reshape(c.N, c.C, -1), t.reshape(c.N, c.C, -1), None if w is None else w.reshape(c.N, w.shape[1], -1),
                         c.pw, rows=(a, b))
    cols = slice(1, 5) if c.family == 2 else slice(0, 5)
    assert bool((tail[:, cols] != 0).all()), f"{c.name}: a sum of the last slot is zero, losing it would not show"
    assert bool(((s - tail)[:, cols] != s[:, cols]).all()) and bool(((s + tail)[:, cols] != s[:, cols]).all())
    # the scalar loss has a derived bound: a lost last slot moves it by more than twice that bound
    den = E.loss_den64(c, s)
    ref = E.loss_ref64(s, den, c.w_bce, c.w_dice, c.snr, c.sdr)
    lost = s - tail
    den_l = E.loss_den64(c, lost)
    bad = E.loss_ref64(lost, den_l, c.w_bce, c.w_dice, c.snr, c.sdr)
    bound = E.gamma(E.LOSS_U) * (c.w_bce * abs(ref[1]) + c.w_dice)
    assert abs(bad[0] - ref[0]) > 2 * bound, (bad[0], ref[0], bound)


def test_an_over_cap_case_fails_on_the_cpu():
    c = E.LossCase("over", 4, 3, (112,) * 3, pw=0.5, wrong=0.9)
    with pytest.raises(AssertionError, match="over the exactness cap"):
        E.loss_assert_caps(c, *E.loss_operands(c))
    c = E.LossCase("fam2", 1, 1, (8, 8, 8), family=2, w_bce=1.0)
    with pytest.raises(AssertionError, match="w_bce must be 0"):
        E.loss_assert_caps(c, *E.loss_operands(c))


def test_slot_emulation_matches_the_shortcut():
    """fp32 slot-split summation (exact_reduction_cases.slot_split_sum_f32) of an exact case equals the fp64 sums, and with the last
    slot dropped / doubled equals the exact sums minus / plus that slot's"""
    c = E.LossCase("emul", 1, 2, (9, 11, 331), pw=0.5)
    x, t, w = E.loss_operands(c)
    s = E.loss_assert_caps(c, x, t, w)
    valid, wb, p = E.loss_terms64(x, t, w, c.pw)
    td = t.double()
    terms = torch.stack([valid * wb, valid, valid * p * td, valid * p, valid * td], -1).reshape(c.N * c.C, c.R, 5).permute(1, 0, 2)
    terms = terms.float().contiguous()
    a, b = X.slot_rows(c.R, c.slots)[-1]
    tail = terms[a:b].double().sum(0)
    assert c.slots == 2 and torch.equal(X.slot_split_sum_f32(terms, c.slots).double(), s)
    assert torch.equal(X.slot_split_sum_f32(terms, c.slots, drop=1).double(), s - tail)
    assert torch.equal(X.slot_split_sum_f32(terms, c.slots, double=1).double(), s + tail)


def _module_loss(x, t, w, pw, wb, wd, snr, sdr):
    from pytorch_connectomics_amd.training import module as M
    xm, tm = M._mask_for_unweighted_loss(x, t, w, -20.0)
    return wb * M.weighted_bce_with_logits(x, t, w, pw) + wd * M.dice_loss_sigmoid(xm, tm, snr, sdr)


@pytest.mark.parametrize("pw,weighted", [(None, False), (0.1, True), (10.0, True)])
def test_fp64_references_agree_with_torch_autograd(pw, weighted):
    """bce_dice_ref64 is training/module.py's formulas (equal to them in fp32 precision, since the module casts to fp32), and
    loss_grad64 with the fp64 sums is torch's double-precision autograd of it"""
    x, t, w = E.clamp_range_operands("uniform", (2, 3, 6, 10, 12), 11)
    w = w if weighted else None
    kw = dict(pw=pw, w_bce=0.75, w_dice=1.5, snr=1e-5, sdr=1e-5)
    xd = x.double().requires_grad_(True)
    loss = E.bce_dice_ref64(xd, t, w, **kw)
    (g,) = torch.autograd.grad(loss, xd)
    m32 = _module_loss(x, t, w, pw, 0.75, 1.5, 1e-5, 1e-5)
    assert abs(float(m32) - float(loss.detach())) < 1e-5 * abs(float(loss.detach()))
    # the kernel's sums (valid voxels only) from fp64 sigmoid: the masked voxels' sigmoid(-20) is all that separates the two
    xf, td = x.double(), t.double()
    valid = torch.ones_like(xf) if w is None else (w.double().expand_as(xf) > 0).double()
    p = torch.sigmoid(xf)
    dims = (2, 3, 4)
    sums = torch.stack([torch.zeros(6, dtype=torch.float64), (valid).sum(dims).reshape(-1), (valid * p * td).sum(dims).reshape(-1),
                        (valid * p).sum(dims).reshape(-1), (valid * td).sum(dims).reshape(-1)], 1)
    den = max(float(valid.sum()), 1.0)
    g2 = E.loss_grad64(x, t, w, sums, den, go=1.0, logistic=True, **kw)
    assert float((g2 - g).abs().max()) < 1e-8 * float(g.abs().max())          # sigmoid(-20) = 2e-9 per masked voxel
    if w is None:
        assert float((g2 - g).abs().max()) < 1e-14 * float(g.abs().max())


def test_exact_family_references_agree_with_torch_double():
    """the analytic p / bce of the exact families against torch double ops on the same logits (sigmoid(+-128) is 1 / 0 to 1e-55)"""
    c = E.LossCase("small", 2, 2, (5, 6, 7), pw=2.0)
    x, t, w = E.loss_operands(c)
    s = E.loss_assert_caps(c, x, t, w)
    den = E.loss_den64(c, s)
    ref = E.loss_ref64(s, den, 1.0, 1.0, 1.0, 1.0)
    full = E.bce_dice_ref64(x, t, w, pw=2.0, w_bce=1.0, w_dice=1.0, snr=1.0, sdr=1.0, clamp_min=-128.0)
    assert abs(ref[0] - float(full)) < 1e-12 * abs(ref[0])
    xd = x.double().requires_grad_(True)
    (g,) = torch.autograd.grad(E.bce_dice_ref64(xd, t, w, pw=2.0, w_bce=1.0, w_dice=1.0, snr=1.0, sdr=1.0, clamp_min=-128.0), xd)
    g2 = E.loss_grad64(x, t, w, s, den, pw=2.0, w_bce=1.0, w_dice=1.0, snr=1.0, sdr=1.0)
    assert float((g - g2).abs().max()) < 1e-12 * float(g.abs().max())


@pytest.mark.parametrize("ema", [False, True])
def test_adamw_reference_is_torch_adamw_in_double(ema):
    g0 = torch.Generator().manual_seed(0)
    p = torch.randn(300, generator=g0, dtype=torch.float64)
    q = torch.nn.Parameter(p.clone())
    opt = torch.optim.AdamW([q], lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    m, v, e = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    for t in range(1, 5):
        g = torch.randn(300, generator=g0, dtype=torch.float64)
        coef = 0.5 if t == 2 else 1.0                   # a clip coefficient scales the gradient torch sees
        q.grad = g * coef
        opt.step()
        r = E.adamw_ref64(p, m, v, g, coef, E.adamw_row(3e-3, (0.9, 0.999), 1e-8, 0.05, t, 0.99, rounded=False),
                          ema=e if ema else None)
        p, m, v = r["p"][0], r["m"][0], r["v"][0]
        if ema:
            want = 0.99 * e + 0.01 * p
            assert torch.allclose(r["ema"][0], want, rtol=1e-14, atol=0)
            e = r["ema"][0]
        assert torch.allclose(p, q.detach(), rtol=1e-12, atol=1e-15)
        assert bool((r["p"][1] > 0).all()) and bool((r["p"][1] < 1e-5 * (p.abs() + 1e-3)).all())
    # fp32 rounding of the row: 1 - beta is exact in fp32 (Sterbenz), so the kernel's (1 - b) equals the row's in double
    row = E.adamw_row(1e-3, (0.9, 0.999), 1e-8, 0.01, 3, 0.999)
    for b in (row[1], row[2], row[7]):
        assert float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(b, dtype=torch.float32)) == 1.0 - b


def test_optimizer_sets_and_chunk_counts():
    assert [E.opt_chunks(n) for n in E.BOUNDARY_LENGTHS] == [1, 1, 1, 2, 2, 2, 3, 4]
    s = E.model_shapes("S")
    nS = [int(torch.Size(x).numel()) for x in s]
    assert len(s) == 229 and sum(nS) == 5550882 and sum(E.opt_chunks(n) for n in nS) == 1509
    assert 1 in nS and any(n % E.OPT_CHUNK for n in nS) and any(n % E.OPT_CHUNK == 0 for n in nS)
    X.assert_exact_cap(sum(nS), 1.0, what="MedNeXt-S sum g^2 of a dense ternary gradient")
    L = [int(torch.Size(x).numel()) for x in E.model_shapes("L")]
    assert len(L) == 517 and sum(L) == 61779234 and sum(E.opt_chunks(n) for n in L) == 15400
    X.assert_exact_cap(sum(L) / 8 * 1.05, 1.0, what="MedNeXt-L sum g^2 at density 1/8")


def test_cldice_caps():
    """the tile-partial sums stay under the cap for the largest case: every voxel a skeleton voxel of weight 2 on a target voxel is
    16 quanta of 1/4"""
    for name, shape, _ in E.CLDICE_SUM_CASES:
        V = int(torch.Size(shape[2:]).numel())
        assert E.cldice_tiles(V) == -(-V // 1024)
        # drawn operands: the GPU case asserts the cap on its own skeleton; here the shape-level bound with the skeleton at most
        # half of the volume (a skeleton voxel has a non-skeleton neighbour along its thinnest axis)
        X.assert_exact_cap(0.5 * V * 4.0 * (0.25 + 1 + 4) / 4, 0.25, what=name)
    assert E.cldice_tiles(112 ** 3) == 1372 and E.cldice_tiles(33 * 47 * 41) == 63 and (33 * 47 * 41) % 1024 == 103


def _lib():
    from pytorch_connectomics_amd import _native as nat
    if not nat.LIB_PATH.exists():
        pytest.skip(f"HIP library {nat.LIB_PATH} not built")
    return nat.lib()


def test_mirrors_match_the_library_queries():
    lib = _lib()
    assert lib.pytc_opt_chunk_elems() == E.OPT_CHUNK
    for R in (1, 5940, 16383, 16384, 32767, 32768, 32769, 112 ** 3, 160 ** 3, 256 * 16384 - 1, 256 * 16384, 170 * 168 * 168, 2 ** 31):
        for N, C in ((1, 1), (4, 3)):
            assert lib.pytc_bce_dice_ws_elems(N, C, R) == E.loss_ws_elems(N, C, R), R
    for c in CASES:
        assert lib.pytc_bce_dice_ws_elems(c.N, c.C, c.R) == c.slots * c.N * c.C * 5
    for V in (1, 1023, 1024, 1025, 112 ** 3, 1024 * 768, 33 * 47 * 41):
        assert lib.pytc_cldice_tiles(V) == E.cldice_tiles(V)

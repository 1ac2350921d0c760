"""CPU checks of the exact-reduction case generator (tests/exact_reduction_cases.py): the operands are exact in bf16, the exactness
caps hold for every listed shape, GELU of the chosen pre-activations is exact under each GELU form the kernels evaluate, and a slot-split
fp32 sum of such terms equals fp64 exactly -- and stops doing so when a slot is dropped or doubled.  With the library built, the slot
mirrors agree with the dispatchers' host-side slot queries."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import exact_reduction_cases as X  # noqa: E402


def test_generated_values_are_exact_in_bf16():
    t = X.ternary((4, 3000, 32), 0.25, 1)
    assert t.dtype == torch.bfloat16 and set(torch.unique(t.float()).tolist()) == {-1.0, 0.0, 1.0}
    frac = float((t != 0).float().mean())
    assert 0.23 < frac < 0.27
    assert X.is_bf16_exact(X.ternary((1000, 8), 0.5, 2, scale=0.5, dtype=torch.float32))
    b = X.binary((1000, 16), 0.5, 3, value=16.0)
    assert set(torch.unique(b.float()).tolist()) == {0.0, 16.0}
    ab = X.exact_affine(5, 64, 4)
    assert set(ab[:, 0].abs().unique().tolist()) <= {0.5, 1.0, 2.0} and set(ab[:, 1].unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    x = X.ternary((5, 100, 64), 0.5, 5).float()
    xn = x * ab[:, 0][:, None] + ab[:, 1][:, None]
    assert X.is_bf16_exact(xn)                                  # the norm affine survives the bf16 rounding of the forward
    assert torch.equal(torch.addcmul(ab[:, 1][:, None], x, ab[:, 0][:, None]), xn)      # fma or not: same values
    dens = X.tail_dense_rows(1000, 10, 1 / 64)
    t = X.ternary((1000, 32), 1.0, 6, row_density=dens)
    assert bool((t[-10:] != 0).all()) and float((t[:-10] != 0).float().mean()) < 0.05


def test_seeded_generation_is_reproducible():
    assert torch.equal(X.ternary((64, 32), 0.5, 9), X.ternary((64, 32), 0.5, 9))
    assert not torch.equal(X.ternary((64, 32), 0.5, 9), X.ternary((64, 32), 0.5, 10))


@pytest.mark.parametrize("c", X.pw_cases(), ids=lambda c: c.name)
def test_pw_caps_hold_for_every_listed_shape(c):
    bound, quantum = X.pw_case_abs_bound(c)
    X.assert_exact_cap(bound, quantum, what=c.name)
    X.assert_exact_cap(c.N * c.rows, 1.0, what=c.name + " db")
    assert c.slots > 1


@pytest.mark.parametrize("c", X.dw_cases(), ids=lambda c: c.name)
def test_dw_caps_and_slots_for_every_listed_shape(c):
    X.assert_exact_cap(c.N * c.gdims[0] * c.gdims[1] * c.gdims[2], 1.0, what=c.name)      # |g x| <= 1 per position and tap
    for m, v in ((1, 1), (0, 1), (0, 0)):
        assert X.dw_wgrad_slots(c.N, c.gdims, c.xdims, c.C, 3, c.stride, march=bool(m), vec=bool(v)) > 1


def test_the_case_lists_cover_ragged_and_straddling_splits():
    facts = [X.split_facts(c.rows, c.N, c.slots) for c in X.pw_cases()]
    assert any(f["ragged"] for f in facts) and any(f["straddle"] for f in facts)
    assert any(f["ragged"] and f["straddle"] for f in facts)
    assert any(c.ab and X.split_facts(c.rows, c.N, c.slots)["straddle"] for c in X.pw_cases())     # per-sample affine across samples
    assert max(c.slots for c in X.pw_cases()) == 1024                                             # the slot cap is reached
    assert {lv for lv, _, _ in X.mednext_levels()} == {0, 1, 2, 3, 4}
    kinds = {(c.kind, X.dw_wgrad_form(c.gdims, c.xdims, c.C, 3, c.stride)) for c in X.dw_cases()}
    assert {("block", "march"), ("block", "vec"), ("down", "vec"), ("up", "vec")} <= kinds


@pytest.mark.parametrize("form", sorted(X.GELU_FORMS))
def test_gelu_exact_values_under_each_form(form):
    f = X.GELU_FORMS[form]
    v = torch.tensor(X.GELU_EXACT_VALUES, dtype=torch.float32)
    g = f(v)
    assert torch.equal(g.bfloat16().float(), v), f"{form}: gelu{tuple(v.tolist())} = {tuple(g.tolist())}"
    assert torch.equal(g, v)                                     # exact in fp32 already
    # the restatements are GELU: against torch's erf form away from the exact points
    u = torch.linspace(-6, 6, 241)
    assert float((f(u) - torch.nn.functional.gelu(u)).abs().max()) < 5e-5


def test_gelu_fast_derivative_is_exact_at_the_chosen_values():
    """mixer_bwd_rc forms dhp = (W3^T dy) gelu'(hp) with gelu_fast_with_grad: its derivative is exactly 1/2 at 0 and 1 at 16"""
    v = torch.tensor(X.GELU_EXACT_VALUES, dtype=torch.float32)
    g, gd = X.gelu_fast_with_grad_f32(v)
    assert torch.equal(g, v) and torch.equal(gd, torch.tensor([0.5, 1.0]))
    u = torch.linspace(-6, 6, 241, requires_grad=True)
    torch.nn.functional.gelu(u).sum().backward()
    assert float((X.gelu_fast_with_grad_f32(u.detach())[1] - u.grad).abs().max()) < 2e-4


@pytest.mark.parametrize("rows,slots", [(1000, 7), (4096, 64), (999, 10), (257, 9)])
def test_slot_split_sum_is_exact_and_sees_a_lost_or_doubled_slot(rows, slots):
    x = X.ternary((rows, 24), 0.5, rows, dtype=torch.float32)
    a = X.exact_affine(1, 24, rows)[0]
    dy = X.ternary((rows, 1), 0.5, rows + 1, dtype=torch.float32)
    terms = dy * (x * a[0] + a[1])                          # multiples of 1/2
    X.assert_exact_cap(float(terms.abs().sum(0).max()), 0.5)
    exact = terms.double().sum(0)
    got = X.slot_split_sum_f32(terms, slots)
    assert torch.equal(got.double(), exact)
    # any other grouping gives the same bits
    assert torch.equal(X.slot_split_sum_f32(terms, max(1, slots // 3)), got)
    last = len(X.slot_rows(rows, slots)) - 1
    lost = X.slot_split_sum_f32(terms, slots, drop=last)
    doubled = X.slot_split_sum_f32(terms, slots, double=last)
    a0, b0 = X.slot_rows(rows, slots)[last]
    tail = terms[a0:b0].double().sum(0)
    assert torch.equal(lost.double(), exact - tail) and torch.equal(doubled.double(), exact + tail)
    assert bool((tail != 0).any()), "the last slot must carry signal for the fault to show"


def test_slot_split_sum_of_inexact_terms_is_not_order_free():
    """the counter-example the exact operands avoid: random fp32 terms round differently per grouping, within the derived bound"""
    t = torch.randn(4096, 8, generator=torch.Generator().manual_seed(0))
    a, b = X.slot_split_sum_f32(t, 64), X.slot_split_sum_f32(t, 4)
    assert not torch.equal(a, b)
    exact = t.double().sum(0)
    bound = X.slot_rounding_bound(64, 64, t.double().abs().sum(0))
    assert bool(((a.double() - exact).abs() <= bound).all())


def test_split_facts():
    f = X.split_facts(100, 3, 7)                            # 300 rows, 43 per slot: last 42, slot 2 spans rows 86..128
    assert f["slots"] == 7 and f["rows_per_slot"] == 43 and f["ragged"] and f["straddle"]
    f = X.split_facts(256, 4, 8)
    assert not f["ragged"] and not f["straddle"]


def _lib():
    from pytorch_connectomics_amd import _native as nat
    if not nat.LIB_PATH.exists():                           # the library is not built: nothing to compare the mirrors with
        pytest.skip(f"HIP library {nat.LIB_PATH} not built")
    return nat, nat.lib()


def test_slot_mirrors_match_the_library_queries():
    nat, lib = _lib()
    from pytorch_connectomics_amd.hip_ops import _i3
    for rows in (1, 255, 256, 5000, 4 * 112 ** 3, 7 ** 3 * 4):
        assert lib.pytc_pw_wgrad_slots(rows) == X.pw_wgrad_slots(rows)
        assert lib.pytc_channel_stats_slots(rows) == X.colstats_slots(rows)
        assert lib.pytc_layernorm_wide_bwd_slots(rows) == X.layernorm_wide_slots(rows)
        assert lib.pytc_layernorm_any_bwd_slots(rows) == X.layernorm_any_slots(rows)
        for C in (48, 96, 32, 128, 256):
            assert lib.pytc_layernorm_rows_bwd_slots(rows, C, nat.BF16) == X.layernorm_rows_slots(rows, C)
    for c in X.dw_cases():
        assert lib.pytc_dw_wgrad_slots(c.N, _i3(c.gdims), _i3(c.xdims), c.C, 3, c.stride, nat.BF16) == \
            X.dw_wgrad_slots(c.N, c.gdims, c.xdims, c.C, 3, c.stride), c.name
    for N, rows, c_hid in ((4, 112 ** 3, 64), (3, 33 * 47 * 61, 64), (5, 16 * 80 * 48, 96)):
        assert lib.pytc_mixer_bwd_rc_sps(N, rows, c_hid) == X.mixer_bwd_rc_sps(N, rows, c_hid)
    for N, rows, C, c_hid in ((4, 112 ** 3, 32, 64), (4, 14 ** 3, 256, 512), (3, 33 * 47 * 61, 32, 64)):
        assert lib.pytc_pw_wgrad_groupnorm_sps(N, rows, C, c_hid) == X.pw_wgrad_groupnorm_sps(N, rows, C, c_hid)
    for rows, ci, cu in ((2 * 32 * 64 * 64, 64, 64), (2 * 4 * 8 * 8, 512, 256), (2 * 216, 768, 128), (16 * 32 * 32, 16, 16)):
        assert lib.pytc_upcat_deconv2_wgrad_ws_elems(rows, ci, cu, nat.BF16) == X.upcat_wgrad_splits(rows, ci, cu) * (ci + 1) * 8 * cu

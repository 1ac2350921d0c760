"""Host proof for tests/test_gpu_layernorm_exact.py (no GPU): the launch rules that tests/layernorm_exact_cases.py restates are the ones
in the sources; every case's exact rows meet their premises in numpy fp32 (exact_rows asserts them: mean = mu, var = a^2,
1 / sqrtf(var) = 1 / a in two summation orders, whole multiples of C, bf16 numbers) and the fp64 formulas give the closed form; every
defect of the list changes a stored output of the exact rows by at least 100 x the largest rsqrt bound; the general-row bounds stay
far below one storage ulp's worth of a wrong chunk; and the table reaches the edges it claims."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import layernorm_exact_cases as X  # noqa: E402
import exact_reduction_cases as R  # noqa: E402

CSRC = Path(__file__).resolve().parents[1] / "pytorch_connectomics_amd" / "csrc"


def test_restated_launch_rules_follow_the_sources():
    wide = (CSRC / "transformer_kernels.hip").read_text()
    mv, rb = map(int, re.search(r"constexpr int LN_MAXV = (\d+), LN_ROWS_PER_BLOCK = (\d+);", wide).groups())
    assert (mv, rb) == (X.WIDE_MAX_CHUNKS, X.WIDE_BWD_ROWS)
    assert "const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);" in wide and X.WIDE_FWD_ROWS == 4
    assert wide.count("rsqrtf(wave_sum(q) / (float)C + eps)") == 2
    swin = (CSRC / "swin_kernels.hip").read_text()
    assert int(re.search(r"constexpr int LNA_ROWS_PER_SLOT = (\d+);", swin).group(1)) == X.ANY_SLOT_ROWS
    assert f"C >= {X.ANY_MIN_C} && C <= {X.ANY_MAX_C} && C % 16 == 0" in swin and "rstd = rsqrtf(wave_sum(q) / (float)C + eps);" in swin
    assert swin.count("const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);") >= 2 and X.ANY_ROWS == 4
    fwd = (CSRC / "norm_pool_kernels.hip").read_text()
    bwd = (CSRC / "norm_variant_kernels.hip").read_text()
    rule = "if (C % v == 0 && pow2(C / v) && C / v <= 64)"
    assert rule in fwd and rule in bwd and "for (int v = 8; v >= 1; v >>= 1)" in fwd and "for (int v = 8; v >= 1; v >>= 1)" in bwd
    assert f"if (blocks > {X.ROWS_FWD_MAX_BLOCKS}) blocks = {X.ROWS_FWD_MAX_BLOCKS};" in fwd
    assert f"return blocks > {X.ROWS_BWD_MAX_BLOCKS} ? {X.ROWS_BWD_MAX_BLOCKS} : blocks;" in bwd
    assert "const float rstd = 1.0f / sqrtf(q / (float)C + eps);" in fwd and "const float rstd = 1.0f / sqrtf(q * inv_c + eps);" in bwd
    assert {C: X.ln_vec(C) for C in X.ROWS_C} == {1: 1, 2: 2, 4: 4, 8: 8, 32: 8, 128: 8, 512: 8}
    assert all(X.ln_vec(C) == 0 for C in X.ROWS_REFUSED)
    assert all(R.layernorm_rows_rpb(C) == X.rows_rpb(C) for C in X.ROWS_C)


def test_exactness_facts_of_the_issue_hold_in_fp32():
    """(C, a, mu) = (48, 2, 3), (768, 4, -5), (6144, 1, 7), (80, 8, 1): mean = mu, var = a^2, 1 / sqrtf(var) = 1 / a; not with eps = 1e-5"""
    f = np.float32
    with_eps = []
    for C, a, mu in ((48, 2, 3), (768, 4, -5), (6144, 1, 7), (80, 8, 1)):
        x = (mu + a * np.where(np.arange(C) % 2, -1.0, 1.0)).astype(f)
        s = f(0)
        for v in x:
            s = f(s + v)
        mean = f(s / f(C))
        q = f(0)
        for v in x:
            q = f(q + f(v - mean) * f(v - mean))
        var = f(q / f(C))
        assert (float(mean), float(var), float(f(1) / np.sqrt(var))) == (mu, a * a, 1 / a)
        with_eps.append(float(f(1) / np.sqrt(f(var + f(1e-5)))) == 1 / a)
    assert not all(with_eps)                                  # eps = 1e-5 breaks it (where a^2 + eps is not a^2 in fp32): hence eps = 0


@pytest.mark.parametrize("c", X.cases(), ids=X.ids(X.cases()))
def test_case_premises_discrimination_and_bounds(c):
    d = X.exact_rows(c)                                       # asserts the premises
    assert d["x"].shape == (c.rows, c.C) and (d["eps"] == 0.0 or c.C == 1)
    found = X.discrimination(c)
    assert found or c.C == 1 and c.rows % X.rows_rpb(1) == 0, c.id
    for key, (change, over_bound) in found.items():
        assert change > 0 and over_bound >= 100, f"{c.id}: the defect {key} moves an output by {change:.3g}, {over_bound:.3g} x the rsqrt bound"
    gd = X.general_rows(c)
    y, dx, By, Bdx = X.general_bounds(c, gd)
    assert np.isfinite(By).all() and np.isfinite(Bdx).all()
    # where a row's variance is at least 1 (rstd does not magnify the mean's rounding) the derived bounds are at most a fifth of the
    # whole-tensor tolerances they replace (1e-4 in fp32) and half of it in bf16 (3e-2), per element and relative to the row's largest
    ok = gd["x"].var(1) >= 1.0
    if ok.any():
        cap = 2e-5 if c.dt == "f32" else 2.0 ** -6
        assert float((By / np.abs(y).max(1, keepdims=True).clip(1))[ok].max()) <= cap
        assert float((Bdx / np.abs(dx).max(1, keepdims=True).clip(1))[ok].max()) <= cap


def test_table_reaches_every_edge_it_claims():
    cs = X.cases()
    for dt in ("bf16", "f32"):
        w = [c for c in cs if c.form == "wide" and c.dt == dt]
        assert {c.C for c in w} == {64, 192, 768, 1024} and {c.rows for c in w} == {1, 3, 4, 5, 31, 32, 33, 65} and 1024 == 64 * X.WIDE_MAX_CHUNKS
        a = [c for c in cs if c.form == "any" and c.dt == dt]
        assert {c.C for c in a} == {16, 48, 80, 96, 1536, 6144} and {c.rows for c in a} == {1, 3, 4, 5, 257} and 257 > X.ANY_SLOT_ROWS
        assert {c.affine for c in a} == {True, False}
        r = [c for c in cs if c.form == "rows" and c.dt == dt and c.kind == "pair"]
        assert {c.C for c in r} == set(X.ROWS_C)
        for C in X.ROWS_C:
            rpb = X.rows_rpb(C)
            assert {c.rows for c in r if c.C == C} == {1, rpb - 1, rpb, rpb + 1} - {0}
        cap = [c for c in cs if c.kind == "bwd_cap" and c.dt == dt]
        assert len(cap) == 1 and -(-cap[0].rows // X.rows_rpb(cap[0].C)) == X.ROWS_BWD_MAX_BLOCKS + 1
    f = X.fwd_cap_case()
    assert (f.dt, f.C, f.rows) == ("bf16", 512, 262145) and -(-f.rows // X.rows_rpb(512)) == X.ROWS_FWD_MAX_BLOCKS + 1
    assert len({c.id for c in cs}) == len(cs)

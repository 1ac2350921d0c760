"""Host proof for tests/test_gpu_pw_conv_exact.py (no GPU): gelu_erf_grad is exact where the cases use it; every filed case meets its
exactness premises (operands are numbers of their types, every output's terms are multiples of one unit 2^-k with sum |terms| below
2^24 units) and discriminates -- each mutation of the reference that a wrong kernel could compute changes at least one stored output;
the case table reaches every kernel instance and edge it claims, with the dispatch restated from the launch code; and the weight-image
models are permutations with zero padding."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import pw_conv_exact_cases as X  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pytorch_connectomics_amd" / "csrc"


# ------------------------------------------------------------------------------------------------------------- GELU
def test_gelu_erf_grad_is_exact_at_the_points_the_cases_store():
    """1/2 at 0, 1 at +16, 0 at -16: at |x| = 16 the exponential 2^(-128 log2 e) underflows to 0, at 0 the polynomial is 1 at t = 1"""
    x = torch.tensor(list(X.GELU_GRAD_EXACT), dtype=torch.float32)
    g = X.gelu_erf_grad_f32(x)
    assert g.dtype == torch.float32 and g.tolist() == list(X.GELU_GRAD_EXACT.values())
    assert g.view(torch.int32).tolist() == torch.tensor([0.5, 1.0, 0.0]).view(torch.int32).tolist()          # +0, not -0
    az = x.abs() * torch.tensor(0.70710678118654752440)
    assert torch.exp2(-az * az * torch.tensor(1.44269504088896340736))[1:].tolist() == [0.0, 0.0]
    # away from these points the function is not exact: the restatement follows the erf derivative to fp32 accuracy
    xs = torch.linspace(-6, 6, 241)
    want = torch.autograd.functional.jacobian(lambda v: torch.nn.functional.gelu(v.double()).sum(), xs.double())
    assert float((X.gelu_erf_grad_f32(xs).double() - want).abs().max()) < 5e-7


def test_gelu_restatements_follow_the_source():
    """the constants of gelu_erf_grad in csrc/pytc_common.h are the restatement's; the forward forms are imported, not copied"""
    src = (CSRC / "pytc_common.h").read_text()
    body = src[src.index("float gelu_erf_grad(float x)"):src.index("Sigmoid-form GELU")]
    for lit in ("0.70710678118654752440f", "0.3275911f", "1.061405429f", "-1.453152027f", "1.421413741f", "-0.284496736f", "0.254829592f",
                "1.44269504088896340736f", "0.3989422804014327f"):
        assert lit in body, lit
    import exact_reduction_cases as R
    assert X.gelu_erf_f32 is R.gelu_erf_f32 and X.gelu_fast_f32 is R.gelu_fast_f32 and X.GELU_EXACT_VALUES is R.GELU_EXACT_VALUES
    for v in X.GELU_EXACT_VALUES:
        for f in (X.gelu_erf_f32, X.gelu_fast_f32):
            assert float(f(torch.tensor([v]))[0]) == v


# ------------------------------------------------------------------------------------------------------------- every case
@pytest.mark.parametrize("c", X.all_cases(), ids=X.ids(X.all_cases()))
def test_case_premises_and_discrimination(c):
    ref = X.assert_premises(c)
    assert ref["worst_units"] < 2.0 ** X.EXACT_BITS
    assert tuple(ref["y"].shape) == c.out_shape and ref["y"].dtype == X.TORCH_DT[c.dt[2]]
    assert torch.isfinite(ref["y"].float()).all()
    app, found = X.applicable(c), X.discrimination(c)
    for name, on in app.items():
        if on:
            assert found.get(name, 0) > 0, f"{c.id}: the mutation '{name}' changes no stored output ({found})"
    print(f"{c.id}: {X.family(c)}, unit 2^{ref['unit_exp']}, sum |terms| <= {ref['worst_units']:.0f} units; changed outputs {found}")
    if c.res in ("up", "up_low"):                           # the front faces equal the skip alone
        face = X.upsample_parts(c.grid)[0]
        d = X.operands(c)
        assert face.any() and torch.equal(ref["y"][:, face], X.to_out(c, d["res"][:, face]))
    if c.ab:
        ab = X.operands(c)["ab"]
        assert all((ab[n] != ab[0]).any() for n in range(1, c.N)), "the affine must differ per sample"
    if "coef" in X.operands(c):
        cf = X.operands(c)["coef"]
        assert all((cf[n] != cf[0]).any() for n in range(1, c.N))


# ------------------------------------------------------------------------------------------------------------- the table
def _instances(form):
    return {X.expected_instance(c) for c in X.cases(form)}


def test_generic_cases_reach_every_instance_and_edge():
    cs = X.cases("generic")
    inst = {X.expected_instance(c) for c in cs}
    want = {f"pw_conv_kernel<{ti}, {tw}, {to}, {mt}, 4>" for ti, tw, to in X.GENERIC_ROUTES for mt in (1, 2, 4)}
    assert inst == want, sorted(want - inst)
    assert {3, 12, 13, 40, 80} <= {c.cout for c in cs} and set(X.GENERIC_ROWS) <= {c.rows for c in cs}
    assert all(c.N == 3 for c in cs)
    for tw, tails in (("bf16", {1, 13, 24, 48}), ("f32", {1, 13, 20})):
        assert tails <= {c.cin for c in cs if c.dt[1] == tw}, tw
    assert all(not c.plain for c in cs if c.cin == 1 and c.dt[1] == "bf16" and c.dt[2] == "bf16")
    f2b = [c for c in cs if c.dt == ("f32", "bf16", "bf16")]
    assert any(c.ab for c in f2b) and any(not c.ab and not c.pre_gelu for c in f2b)               # the operand rounding, with and without ab
    for rt in X.GENERIC_ROUTES:
        mine = [c for c in cs if c.dt == rt]
        assert any(c.ab for c in mine) and any(c.act == "gelu" for c in mine) and any(c.pre_gelu for c in mine), rt
        assert any(c.res == "add" for c in mine) and any(not c.bias for c in mine), rt
    assert {c.gather for c in cs if c.gather} == {(5, 6, 7), (1, 1, 1), (2, 1, 3)}
    ups = {(c.res, c.res_bias) for c in cs if c.grid}
    assert ups == {("up", True), ("up", False), ("up_low", True), ("up_low", False)} and all(c.grid == (2, 4, 6) for c in cs if c.grid)
    assert any(c.res == "gelu_bwd" for c in cs)


def test_thin_cases_reach_both_kernels_their_edges_and_their_fallbacks():
    stem, head = X.cases("stem"), X.cases("head")
    on = {X.expected_instance(c) for c in stem}
    assert {"pw_stem_kernel<f32>", "pw_stem_kernel<bf16>"} <= on
    assert {c.cout for c in stem if X.expected_instance(c).startswith("pw_stem")} == {8, 32, 256}
    assert all(X.expected_instance(c).startswith("pw_conv_kernel") for c in stem if c.cout == 24)
    assert all(X.expected_instance(c, thin=0).startswith("pw_conv_kernel") for c in stem + head)
    trips = {c.name: X.stem_blocks(c) for c in stem if c.cout % 8 == 0 and 256 % (c.cout // 8) == 0}
    assert trips["f32-256-above-cap"] == (X.STEM_MAX_BLOCKS, 2) and trips["bf16-256-at-cap"] == (X.STEM_MAX_BLOCKS, 1)
    assert all(v[1] == 1 for k, v in trips.items() if "cap" not in k)
    assert any((c.N * c.rows) % (256 // (c.cout // 8)) for c in stem if c.cout in (8, 32, 256))
    assert {X.expected_instance(c) for c in head if c.cin in (8, 64, 512)} == {"pw_head_kernel<bf16>", "pw_head_kernel<f32>"}
    assert all(X.expected_instance(c).startswith("pw_conv_kernel") for c in head if c.cin in (24, 1024))
    assert {c.N * c.rows for c in head} == {1, 7, 513}
    src = (CSRC / "pw_kernels.hip").read_text()
    assert f"ceil_div(work, 256) : {X.STEM_MAX_BLOCKS})" in src and "a->C_in <= 512" in src


def test_paired_cases_reach_every_instance_split_and_epilogue():
    cs = X.cases("paired")
    assert all(X.paired_supported(c) for c in cs)
    for ks, nt in X.PAIRED_NT.items():
        mine = [c for c in cs if c.cin == 32 * ks]
        wg = 4 * nt * 16
        assert any(c.rows % (nt * 16) and c.rows % wg <= wg - nt * 16 and c.rows > wg for c in mine), f"KS {ks}: no tail with idle waves"
        assert any(c.rows == 1 for c in mine)
    by = {c.name: X.paired_zsplit(c) for c in cs}
    assert by["32-256-z8"] == 8 and by["64-192-z2"] == 2 and by["128-96-z1"] == 1 and by["32-64-512-row-blocks"] == 1
    assert any(c.cout == 32 and X.paired_zsplit(c) == 1 for c in cs)
    big = next(c for c in cs if c.name == "32-64-512-row-blocks")
    assert -(-big.rows // 256) * big.N == 512 and (big.cout // 32) % 2 == 0
    src = (CSRC / "pw_fast_kernels.hip").read_text()
    assert "row_blocks * zsplit < 512 && (p.C_out / 32) % (zsplit * 2) == 0" in src
    nts = dict((int(a), int(b)) for a, b in re.findall(r"case (\d+): launch_fast<\d+, (\d)>", src))
    nts[32] = int(re.search(r"default: launch_fast<32, (\d)>", src).group(1))
    assert nts == X.PAIRED_NT
    assert {c.res for c in cs} == {"none", "add", "gelu_bwd", "norm_bwd", "norm_bwd_crop", "up", "up_low"}
    assert {(c.res, c.res_bias) for c in cs if c.res in ("up", "up_low")} == {("up", True), ("up", False), ("up_low", True), ("up_low", False)}
    assert any(c.gather and c.gather[0] % 2 and c.gather[2] % 2 for c in cs) and any(c.ab for c in cs) and any(c.pre_gelu for c in cs)
    assert any(not c.bias for c in cs) and any(c.bias for c in cs)
    assert all(c.N >= 2 for c in cs if c.ab or "norm_bwd" in c.res)


def test_rowmajor_cases_reach_all_four_instances_on_both_sides_of_the_switch():
    cs = X.cases("rowmajor")
    assert all(X.rowmajor_supported(c) for c in cs)
    assert _instances("rowmajor") == {f"pw_gemm_lds_kernel<false, {br}, {ks}, true>" for br in (64, 128) for ks in (32, 64)}
    tiles = {c.name: -(-c.N * c.rows // 128) * (c.cout // 128) for c in cs}
    assert tiles["64-1024-r8064-ab-add"] == 504 and tiles["64-1024-r8065-ab-norm_bwd"] == 512
    for c in cs:
        br = 128 if "128," in X.expected_instance(c) else 64
        assert any(n * c.rows % br for n in range(1, c.N)), f"{c.id}: no tile straddles a sample boundary"
    src = (CSRC / "pw_gemm_kernels.hip").read_text()
    assert "tiles128 >= 512" in src and "a->C_in <= 512" in src
    assert {c.res for c in cs} >= {"add", "gelu_bwd", "norm_bwd", "norm_bwd_crop", "up", "up_low"} and any(c.pre_gelu for c in cs)
    assert any(c.ab and "norm_bwd" in c.res for c in cs)


def test_ids_name_form_and_edge_and_buffers_stay_small():
    for c in X.all_cases():
        assert c.id.startswith(c.form + "-") and c.edge
        esz = {"bf16": 2, "f32": 4}
        assert c.N * c.rows_in * c.cin * esz[c.dt[0]] <= 64 << 20 and int(np.prod(c.out_shape)) * esz[c.dt[2]] <= 64 << 20, c.id


# ------------------------------------------------------------------------------------------------------------- weight images
@pytest.mark.parametrize("tw", ["bf16", "f32"])
def test_packed_image_model_is_a_permutation_with_zero_padding(tw):
    for cout, cin in ((13, 20), (40, 48), (1, 64), (32, 1)):
        w = np.arange(1, cout * cin + 1, dtype=np.float64).reshape(cout, cin)
        img = X.packed_model(w, tw)
        assert len(img) == X.packed_elems_model(cout, cin, tw)
        assert sorted(img[img != 0].tolist()) == w.reshape(-1).tolist() and int((img == 0).sum()) == len(img) - w.size
        # the address formula of packed_weight() in csrc/pw_kernels.hip
        ks, epl = X.KSTEP[tw], X.EPL[tw]
        KG = -(-cin // ks)
        for o, k in ((0, 0), (cout - 1, cin - 1), (cout // 2, cin // 3)):
            kg, kr = divmod(k, ks)
            assert img[(((o // 16) * KG + kg) * 64 + o % 16 + 16 * (kr // epl)) * epl + kr % epl] == w[o, k]


def test_paired_image_model_follows_paired_row():
    w = np.arange(1, 64 * 40 + 1, dtype=np.float64).reshape(64, 40)
    img = X.packed_paired_model(w).reshape(4, 2, 64, 8)
    for T, m, k in ((0, 0, 0), (1, 5, 33), (3, 15, 39), (2, 9, 7)):
        assert img[T, k // 32, m + 16 * (k % 32 // 8), k % 8] == w[X.paired_row(T, m), k]
    assert sorted(X.paired_row(T, m) for T in range(4) for m in range(16)) == list(range(64))

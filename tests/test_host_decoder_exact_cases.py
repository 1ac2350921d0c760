"""Host proof for tests/test_gpu_decoder_exact.py (no GPU): the launch rules that tests/decoder_exact_cases.py restates are the ones in
csrc/upcat_kernels.hip; every filed case meets its exactness premises for the reference alone (operands are numbers of their types,
sum |terms| below 2^24 units, |reference| <= 256 for bf16, the index model equals the fp64 conv_transpose3d + replicate pad + cat and
its autograd); every defect of the list changes at least one stored output of every case it applies to; and the table reaches the
tile, k-step, face and copy-cap edges it claims."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import decoder_exact_cases as X  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pytorch_connectomics_amd" / "csrc"


def test_restated_launch_rules_follow_the_source():
    src = (CSRC / "upcat_kernels.hip").read_text()
    bp, bq = map(int, re.search(r"constexpr int UP_BP = (\d+), UP_BQ = (\d+);", src).groups())
    assert (bp, bq) == (X.UP_BP, X.UP_BQ)
    assert int(re.search(r"constexpr int UP_MAX_ROW_TILES = (\d+);", src).group(1)) == X.MAX_ROW_TILES
    assert "const int wp = wave & 1, wq = wave >> 1;" in src and "(wp * 32 + t * 16 + r16)" in src       # four waves of 32 x 32
    cap = re.search(r"std::min<long>\(\(total \+ (\d+)\) / (\d+), (\d+)\)", src)
    assert (int(cap.group(1)) + 1, int(cap.group(2)), int(cap.group(3))) == (X.COPY_BLOCK, X.COPY_BLOCK, X.COPY_MAX_BLOCKS)
    assert "dim3(grid), dim3(256)" in src
    common = (CSRC / "pytc_common.h").read_text()
    ks = re.search(r"constexpr int mfma_kstep\(int dtype\) \{ return dtype == PYTC_BF16 \? (\d+) : (\d+); \}", common)
    assert (int(ks.group(1)), int(ks.group(2))) == (X.KSTEP["bf16"], X.KSTEP["f32"])
    assert "constexpr int KS = M::KSTEP;" in src
    # P, Q, K of the two GEMMs and their grids; the row tiles are gridDim.y in both, refused by name past the limit
    assert "const int Pdim = MODE == UPCAT_FWD ? Cu8 : (MODE == UPCAT_DGRAD ? p.C_in : p.C_in + 1);" in src
    assert "k_end = MODE == UPCAT_FWD ? p.C_in : (MODE == UPCAT_DGRAD ? Cu8 : p.rows);" in src
    assert src.count("dim3 grid(ceil_div(8L * C_u, UP_BP), ceil_div(p.rows, UP_BQ));") == 2
    assert src.count("dim3 grid(ceil_div(C_in, UP_BP), ceil_div(p.rows, UP_BQ));") == 2
    for entry in ("upcat_deconv2_fwd", "upcat_deconv2_bwd_data", "deconv2_upfirst_fwd", "deconv2_upfirst_bwd_data"):
        assert f'upcat_row_tiles_check("{entry}", N, d, h, wd)' in src
    # placement: the up half at C_e ([skip, up]) or 0 ([up, skip]); the operand roundings of the bf16 route
    assert "p.up_off = C_e; p.Ct = C_e + C_u;" in src and "p.up_off = 0;" in src
    assert "sP[ip * PITCH + kk] = from_f32<T>(pv[q]);" in src and "sQ[ip * PITCH + kk] = from_f32<T>(qv[q]);" in src


def test_the_other_row_tile_launches_refuse_by_name():
    """linear_launch (M tiles) and layernorm_any_param_kernel (row slots) sit on gridDim.y as well"""
    lin = (CSRC / "transformer_kernels.hip").read_text()
    assert "dim3 grid(ceil_div(p.N, LG_BN), ceil_div(p.M, LG_BM));" in lin and "constexpr int LG_MAX_M_TILES = 65535;" in lin
    for entry, m in (("linear_fwd", "M"), ("linear_bwd_data", "M"), ("linear_wgrad", "N")):
        assert f'linear_m_tiles_check("{entry}", {m})' in lin
    swin = (CSRC / "swin_kernels.hip").read_text()
    assert "dim3 pg(ceil_div(C, 256), slots);" in swin and "constexpr int LNA_MAX_SLOTS = 65535;" in swin
    assert "param_slots <= LNA_MAX_SLOTS" in swin


def test_rounding_facts_the_special_cases_rest_on():
    b = lambda v: torch.tensor(v, dtype=torch.float32).to(torch.bfloat16).float().tolist()
    assert b([257.0, 259.0, 261.0]) == [256.0, 260.0, 260.0]
    assert X.store(np.array([257.0, 259.0, 261.0]), "bf16", trunc=True).tolist() == [256.0, 258.0, 260.0]
    assert b([1 + j * 2.0 ** -10 for j in X.WCONV_J]) == [X.WCONV_STAGED[j] for j in X.WCONV_J]
    assert X.store(np.array([1 + j * 2.0 ** -10 for j in X.WCONV_J]), "bf16", trunc=True).tolist() == [X.WCONV_TRUNCATED[j] for j in X.WCONV_J]
    assert all(X.store(np.array([float(v)]), "bf16")[0] == v for v in range(-256, 257))
    cap = next(c for c in X.special_cases() if c.kind == "copycap")
    n = int(np.prod(cap.skip)) * cap.ch[1]
    assert (n, X.COPY_BLOCK * X.COPY_MAX_BLOCKS) == (2230800, 2097152) and X.copy_trips(n) == 2
    assert all(X.copy_trips(int(np.prod(c.skip)) * c.N * c.ch[1]) <= 1 for c in X.all_cases() if c.kind != "copycap")
    assert not X.refused_rows(65535 * 64) and X.refused_rows(65535 * 64 + 1)


@pytest.mark.parametrize("c", X.all_cases(), ids=X.ids(X.all_cases()))
def test_case_premises_and_discrimination(c):
    ref = X.premises(c)
    assert ref["fwd_abs"] / ref["unit"] < 2 ** 24 and ref["dgrad_abs"] / ref["unit"] < 2 ** 24
    assert ref["cat"].shape == (c.N, *c.skip, c.Ct) and ref["dx_low"].shape == (c.N, *c.low, c.ch[0])
    found = X.discrimination(c)
    assert found, c.id
    for key, n in found.items():
        if key[1] == "silent_channels":
            assert n == [], f"{c.id}: losing {key[0]} k index {n} changes no stored output"
        else:
            assert n > 0, f"{c.id}: the defect {key} changes no stored output"


def test_table_reaches_every_edge_it_claims():
    up, first = X.upcat_cases(), X.upfirst_cases()
    for cs in (up, first):
        for dt in ("bf16", "f32"):
            mine = [c for c in cs if c.dt == dt]
            assert {c.ch for c in mine} >= set(X.CHANNELS)
            assert {(c.low, c.N) for c in mine} == {((1, 1, 1), 1), ((2, 3, 5), 1), ((3, 4, 6), 3)}
            assert any(c.bias for c in mine) and any(not c.bias for c in mine)
    assert {c.odd for c in up if c.low == (2, 3, 5) and c.ch == (3, 7, 5) and c.dt == "bf16"} == set(X.ODD8)
    assert any(c.ch[1] == 0 for c in first) and all(c.ch[1] >= 1 for c in up)
    by = {c.ch: c for c in up if c.dt == "bf16" and c.low == (3, 4, 6)}
    f32 = {c.ch: c for c in up if c.dt == "f32" and c.low == (3, 4, 6)}
    # (3, 7, 5): K below one step; 40 columns, parity blocks of 5 cut the 4-column lane groups
    assert X.gemm_dims(by[(3, 7, 5)], "fwd") == (40, 216, 3) and X.k_steps(by[(3, 7, 5)], "fwd") == 1 and 5 % 4
    # (16, 1, 8): exactly one P tile, exactly one fp32 step
    assert X.gemm_grid(by[(16, 1, 8)], "fwd")[0] == 1 and 8 * 8 == X.UP_BP and X.k_steps(f32[(16, 1, 8)], "fwd") == 1
    # (33, 4, 12): one bf16 step + 1; 96 columns: a P tail of 32
    assert X.k_steps(by[(33, 4, 12)], "fwd") == 2 and 33 % 32 == 1 and 96 % X.UP_BP == 32
    # (72, 32, 24): three P tiles; DGRAD K = 192
    assert X.gemm_grid(by[(72, 32, 24)], "fwd")[0] == 3 and X.gemm_dims(by[(72, 32, 24)], "dgrad")[2] == 192
    # (130, 8, 9): DGRAD P = 130, a tail of 2
    assert X.gemm_dims(by[(130, 8, 9)], "dgrad")[0] == 130 and 130 % X.UP_BP == 2
    # rows: 1; 30 (one partial tile); 216 = 3 x 72 (a tail of 24, tiles that straddle samples)
    assert by[(3, 7, 5)].rows == 216 and 216 % 64 == 24 and by[(3, 7, 5)].straddles and 72 % 64
    assert {c.rows for c in up} == {1, 30, 216}
    # 1, 2, 4 and 8 copies of a voxel in the forward / folded terms in the backward, over the eight skip grids
    copies = set()
    for c in up:
        if c.low == (2, 3, 5) and c.ch == (3, 7, 5) and c.dt == "bf16":
            per_row = {}
            for par, _, m, _ in X._targets(c):
                for r in np.nonzero(m)[0]:
                    per_row[(par, r)] = per_row.get((par, r), 0) + 1
            copies |= set(per_row.values())
    assert copies == {1, 2, 4, 8}
    kinds = {c.kind for c in X.special_cases()}
    assert kinds == {"round", "wconv", "copycap"} and all(c.dt == "bf16" for c in X.special_cases())
    assert len({c.id for c in X.all_cases()}) == len(X.all_cases())


# ------------------------------------------------------------------------------------------------------------- B. thin transposed convs
def test_thin_rules_follow_the_source():
    src = (CSRC / "conv3d_strided_kernels.hip").read_text()
    assert int(re.search(r"constexpr int CT_OMAX = (\d+);", src).group(1)) == X.THIN_OMAX
    assert ("return (C_out >= 1 && C_out <= CT_OMAX && C_in >= 8 && C_in % 8 == 0 && (size_t)27 * C_out * C_in * 4 <= 64 * 1024) ? 1 : 0;"
            in src and X.THIN_LDS_BYTES == 64 * 1024)
    cap = re.search(r"long blocks = \(total \+ 255\) / 256;\s*if \(blocks > (\d+)\) blocks = (\d+);", src)
    assert int(cap.group(1)) == int(cap.group(2)) == X.THIN_MAX_BLOCKS and X.THIN_BLOCK == 256
    assert "wl[i] = w[((long)c * C_out + o) * 27 + t];" in src and "wl[i] = w[(long)(i % C_in) * 27 + i / C_in];" in src   # [c][o][t]
    assert src.count("tp[0] = 0; sp[0] = (o + 1) >> 1; tp[1] = 2; sp[1] = (o - 1) >> 1;") == 2
    assert src.count("if (sp[0] >= n_in) tp[0] = -1;") == 2
    ops = (ROOT / "pytorch_connectomics_amd" / "hip_ops.py").read_text()
    assert f"if co == 1 and ci % 8 == 0 and ci <= {X.C1_MAX_CIN}:" in ops
    for (ci, co), want in {(144, 4): True, (600, 1): True, (512, 1): True, (152, 4): False, (608, 1): False, (12, 1): False,
                           (8, 5): False}.items():
        assert X.thin_supported(ci, co) is want, (ci, co)
    assert X.thin_routes(64, 1) == ("c1", "thin") and X.thin_routes(64, 2) == ("thin", "thin") and X.thin_routes(512, 1)[0] == "c1"


THIN_ALL = X.thin_cases() + [X.thin_cap_case()]


@pytest.mark.parametrize("c", THIN_ALL, ids=X.ids(THIN_ALL))
def test_thin_case_premises_and_discrimination(c):
    X.thin_premises(c)
    found = X.thin_discrimination(c)
    assert found and all(n > 0 for n in found.values()), f"{c.id}: defects that change no stored output: {[k for k, n in found.items() if not n]}"


def test_thin_table_reaches_every_edge_it_claims():
    cs = X.thin_cases()
    for dt in ("bf16", "f32"):
        mine = [c for c in cs if c.dt == dt and c.kind == "ternary"]
        assert {(c.cin, c.cout) for c in mine} == set(X.THIN_CHANNELS) and all(X.thin_supported(c.cin, c.cout) for c in mine)
        assert {c.grid for c in mine} == set(X.THIN_GRIDS) and {c.N for c in mine} == {1, 3}
        for ch in X.THIN_CHANNELS:
            assert {(c.N, c.bias) for c in mine if (c.cin, c.cout) == ch} == {(1, True), (1, False), (3, True), (3, False)}
    cap = X.thin_cap_case()
    assert (cap.outputs, X.THIN_MAX_BLOCKS * X.THIN_BLOCK) == (17039360, 16777216) and X.thin_trips(cap.outputs) == 2
    assert all(X.thin_trips(c.outputs) == 1 for c in cs)
    # a one-voxel input: every odd output coordinate loses its tap-0 source
    (t0, s0, v0), (t1, s1, v1) = X._thin_axis(1)
    assert v0.tolist() == [True, False] and v1.tolist() == [False, True] and t1[1] == 2 and s1[1] == 0


# ------------------------------------------------------------------------------------------------------------- C. bilinear up-sampling
def test_depthwise_rules_follow_the_source():
    src = (CSRC / "norm_pool_kernels.hip").read_text()
    assert "constexpr int V = elems_per_16b_of<T>;" in src and "if (C % V == 0)" in src
    common = (CSRC / "pytc_common.h").read_text()
    assert re.search(r"elems_per_16b_of\s*=\s*16\s*/\s*(\(int\))?sizeof\(T\)", common), "elems_per_16b_of is not 16 / sizeof(T)"
    assert X.VEC_ELEMS == {"bf16": 8, "f32": 4}
    assert "if (tz < 0 || tz % g.sz || tz / g.sz >= g.D) continue;" in src                       # the scalar form's remainder test
    assert "for (int kz = (oz + g.pz) % g.sz; kz < g.kd; kz += g.sz)" in src                     # the vector form's tap stride
    for factor, (k, p) in {(1, 2, 2): ((1, 4, 4), (0, 1, 1)), (2, 2, 2): ((4, 4, 4), (1, 1, 1))}.items():
        kk, ss, pp, plane = X.bilinear_geometry(factor)
        assert (kk, ss, pp) == (k, factor, p)
        assert np.array_equal(np.rint(plane * 16), plane * 16) and plane.reshape(k)[0].sum() == 4.0        # multiples of 1/16
    want = {(1, "bf16"): False, (1, "f32"): False, (4, "bf16"): False, (4, "f32"): True, (6, "bf16"): False, (6, "f32"): False,
            (8, "bf16"): True, (8, "f32"): True}
    assert {(C, dt): X.dw_vectorised(C, dt) for C in X.DW_CHANNELS for dt in ("bf16", "f32")} == want


@pytest.mark.parametrize("c", X.dw_cases(), ids=X.ids(X.dw_cases()))
def test_depthwise_case_premises_and_discrimination(c):
    X.dw_premises(c)
    found = X.dw_discrimination(c)
    assert found and all(n > 0 for n in found.values()), f"{c.id}: defects that change no stored output: {[k for k, n in found.items() if not n]}"


def test_depthwise_table_reaches_every_edge_it_claims():
    cs = X.dw_cases()
    for dt in ("bf16", "f32"):
        for geo in ("up122", "up222", "generic"):
            mine = [c for c in cs if c.dt == dt and c.geo == geo]
            assert {c.C for c in mine} == set(X.DW_CHANNELS) and {c.N for c in mine} == {1, 3}
            small = (1, 1, 2) if geo == "generic" else (1, 1, 1)
            assert {c.grid for c in mine} == {small, (2, 3, 5), (3, 6, 7)}
            assert {X.dw_vectorised(c.C, dt) for c in mine} == {True, False}
    # the generic geometry reaches both the % stride and the / stride branches: strides 3, 2 and 1, a kernel longer than its stride
    g = X.DW_GENERIC
    assert g == dict(kernel=(3, 5, 2), stride=(3, 2, 1), pad=(0, 2, 1)) and g["kernel"][1] > g["stride"][1] > 1

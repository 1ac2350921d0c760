"""Exact-arithmetic cases for the single pointwise convolution pytc_pw_conv_fwd (CPU only, numpy + torch):

    y[n][r][o] = epi( act( sum_k q(g(f(x[n][src(r)][k]))) W[o][k] + bias[o] ) )          (include/pytc_hip.h, the pytc_pw_args comment)

f = the per-sample affine a x + b, g = the GELU of `pre_act`, q = the conversion into the MFMA operand (a rounding to bf16 when the
weights are bf16 and the value is not a bf16 number already), src = the stride-2 gather, epi = the residual mode.  Five launch forms
run it: the generic MFMA kernel (pw_conv_kernel, four dtype routes, MT 1 / 2 / 4), the thin stem and head kernels, the paired-row
kernel (pw_fast_kernel, six KS instances, output-channel pairs shared out over blockIdx.z) and the row-major LDS GEMM
(pw_gemm_lds_kernel<false, BR, KS, true>, four instances).  CASES files one case per edge of each form with the instance it expects
(expected_instance restates the dispatch of csrc/pw_kernels.hip, launch_fast and pw_gemm_rowmajor_launch).

Operands (tests/test_host_pw_conv_exact_cases.py proves the premises and the power to discriminate, case by case):

  effective input  three families, after tests/mixer_exact_cases.py.  "sparse": two non-zeros +-1 per row at channels (2g, 2g + 1) mod
           C_in, g the global input row -- every channel and every k step occurs once 2 N rows >= C_in -- against a DENSE weight;
           "dense": integers in [-1, 1] with few zeros against a weight with two non-zeros per output row (every input channel used
           once 2 C_out >= C_in); "full" (the one-channel heads with few rows, where neither covers C_in): +-1 in every channel against
           a dense weight.  Wide-K sums of the first two hold two products, so |y| stays small and one unit survives the bf16 store.
  weights  {+-1/2, +-1, +-(1 + 3/128)} as bf16, {+-1/2, +-1, +-(1 + 2^-9)} as fp32: sums of two leave the bf16 grid, which is what
           separates a truncating store from a rounding one.
  fp32 in  fp32 weights: non-zeros are +-(1 + 2^-9) -- not bf16 numbers, a detour through bf16 shows.  bf16 weights: non-zeros are
           +-(1 + j 2^-10), j in {3, 4, 5, 12}: below, at (ties to even, both parities) and above the midpoint of two bf16 numbers, so
           the rounding of the operand is pinned with and without the affine (fmaf(t, a, b) is exact in fp32, then rounded).
  affine   a in {1/2, 1, 2}, b0 a multiple of 1/2, different per (sample, channel); bf16 inputs add {0, 3, 5} 2^-9 to b, so that
           a t + b is an fp32 number off the bf16 grid and its conversion rounds.
  GELU     has no exact value in general.  pre_act: a t + b in {0, 16}, where gelu_erf, gelu_fast (and so the row-major GEMM's pre_gelu)
           return their argument (exact_reduction_cases.GELU_EXACT_VALUES, proved by its host test).  act = GELU: a one-hot input against
           weights in {0, +-16} and biases in {0, 16} puts every pre-activation on {0, 16}.  RES_GELU_BWD: stored pre-activations in
           {0, +16, -16}, where gelu_erf_grad is exactly 1/2, 1, 0 (gelu_erf_grad_f32 below; the exponential underflows at |x| = 16).
  epilogue operands: quarters of magnitude <= 2; norm-backward coefficients A in {1/2, 1, 2}, B in {-1/2, 1/4, 1/2, 1}, C quarters,
           different per (sample, channel).

Premise, asserted for every output of every case (assert_premises): all terms of its sum -- products, bias, residual, low-resolution
residual, norm-backward terms -- are multiples of one unit 2^-k and sum |terms| < 2^24 units.  Then every partial sum in any order is
an fp32 number; the MFMA sums, the fmaf of the affine and the epilogue adds are exact; the only roundings are q and the store.  The
reference is the fp64 value rounded once to the output type.

NOT covered exactly, left to the tolerance tests of tests/test_gpu_kernels.py: act = PYTC_ACT_SIGMOID / PYTC_ACT_TANH (__expf / tanhf
have no exact point that exercises them) and GELU away from {0, 16}.  pytc_pw_conv_fwd refuses every other activation code
(PYTC_ACT_RELU and its kin belong to the dense convs: apply_act of csrc/pw_common.h never evaluated them).  RES_NORM_BWD exists on the
paired-row and row-major forms only.  The fused wgrad + dgrad kernel and the mixers have suites of their own."""
from __future__ import annotations

import sys
import zlib
from dataclasses import dataclass, fields
from functools import lru_cache
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from exact_reduction_cases import GELU_EXACT_VALUES, _f32, gelu_erf_f32, gelu_fast_f32  # noqa: E402,F401
from mixer_exact_cases import EXACT_BITS, _bf16_bits, bf16_np, check_bits, paired_row, to_bf16  # noqa: E402,F401

KSTEP = {"bf16": 32, "f32": 16}          # Mma<TW>::KSTEP
EPL = {"bf16": 8, "f32": 4}              # Mma<TW>::EPL
TORCH_DT = {"bf16": torch.bfloat16, "f32": torch.float32}
GEMM_KS, GEMM_BN = 64, 128               # csrc/pw_gemm_kernels.hip
STEM_MAX_BLOCKS = 8192                   # pytc_pw_conv_fwd: the stem launch's grid cap
KNOB_DEFAULTS = {"pw_thin": 1}
GELU_GRAD_EXACT = {0.0: 0.5, 16.0: 1.0, -16.0: 0.0}


def gelu_erf_grad_f32(x: torch.Tensor) -> torch.Tensor:
    """fp32 restatement of gelu_erf_grad (csrc/pytc_common.h), in the manner of exact_reduction_cases.gelu_erf_f32"""
    x = x.float()
    az = x.abs() * _f32(0.70710678118654752440)
    t = 1.0 / (_f32(0.3275911) * az + 1.0)
    p = t * _f32(1.061405429) + _f32(-1.453152027)
    p = t * p + _f32(1.421413741)
    p = t * p + _f32(-0.284496736)
    p = t * p + _f32(0.254829592)
    p = p * t
    e = torch.exp2(-az * az * _f32(1.44269504088896340736))
    pe = p * e
    one_plus_erf = torch.where(x < 0, pe, 2.0 - pe)
    return (x * _f32(0.3989422804014327)) * e + 0.5 * one_plus_erf


# ------------------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    form: str                    # generic | stem | head | paired | rowmajor: the launch form the CALL asks for (thin forms: a plain call)
    name: str
    dt: tuple                    # (input, weight, output) of "f32" / "bf16"
    cin: int
    cout: int
    N: int
    rows: int                    # OUTPUT rows per sample (RES_NORM_BWD cropped: the padded grid's rows)
    bias: bool = True
    ab: bool = False
    pre_gelu: bool = False
    act: str = "none"            # none | gelu
    res: str = "none"            # none | add | gelu_bwd | norm_bwd | norm_bwd_crop | up | up_low
    res_bias: bool = True        # RES_UPSAMPLE: the stride holes' bias given
    gather: tuple = ()           # the input grid of gather = 2
    grid: tuple = ()             # RES_UPSAMPLE: the even output grid; norm_bwd_crop: the padded grid
    seed: int = 0                # draws other operands (where a case has one output, the draw decides whether its store rounds)
    edge: str = ""               # what the case is there for

    @property
    def id(self) -> str:
        return f"{self.form}-{self.name}"

    @property
    def data_key(self) -> tuple:
        return tuple(getattr(self, f.name) for f in fields(self) if f.name not in ("name", "edge"))

    @property
    def w_paired(self) -> int:
        return {"paired": 1, "rowmajor": 2}.get(self.form, 0)

    @property
    def plain(self) -> bool:
        return not (self.ab or self.pre_gelu or self.res != "none" or self.gather or self.w_paired)

    @property
    def rows_in(self) -> int:
        return int(np.prod(self.gather)) if self.gather else self.rows

    @property
    def rounds_operand(self) -> bool:
        """the form converts an fp32 value into a bf16 MFMA operand"""
        return self.dt[1] == "bf16" and (self.dt[0] == "f32" or self.ab or self.pre_gelu)

    @property
    def out_shape(self) -> tuple:
        if self.res == "norm_bwd_crop":
            d, h, w = self.grid
            return (self.N, (d - 1) * (h - 1) * (w - 1), self.cout)
        return (self.N, self.rows, self.cout)


def _key_case(key: tuple) -> Case:
    names = [f.name for f in fields(Case) if f.name not in ("name", "edge")]
    return Case(name="data", **dict(zip(names, key)))


def family(c: Case) -> str:
    if c.act == "gelu":
        return "onehot"
    if c.cin == 1 or 2 * c.cout >= c.cin:
        return "dense"
    live = c.rows                                            # rows per sample whose GEMM sum reaches the output
    if c.grid:
        live = int(np.prod([v - 1 for v in c.grid]))         # RES_UPSAMPLE: the front faces take the skip; cropped: they are dropped
    if not c.gather and 2 * c.N * live >= c.cin:
        return "sparse"
    return "full"


# ---- the dispatch of csrc/pw_kernels.hip, restated
def paired_supported(c: Case) -> bool:
    """pw_fast_supported"""
    if c.dt != ("bf16", "bf16", "bf16") or c.cin % 32 or c.cout % 32 or c.act != "none":
        return False
    if c.gather and c.res in ("up", "up_low"):
        return False
    return c.cin // 32 in (1, 2, 4, 8, 16, 32)


def rowmajor_supported(c: Case) -> bool:
    """pw_gemm_rowmajor_supported"""
    return (c.dt == ("bf16", "bf16", "bf16") and c.cin % GEMM_KS == 0 and c.cin >= GEMM_KS and c.cout % GEMM_BN == 0 and c.cout >= GEMM_BN
            and not c.gather and c.act == "none")


PAIRED_NT = {1: 4, 2: 4, 4: 2, 8: 2, 16: 1, 32: 1}           # KS -> NT: pw_fast_launch


def paired_zsplit(c: Case) -> int:
    """launch_fast: output-channel pairs are shared out over blockIdx.z while fewer than 512 workgroups exist"""
    rpb = 4 * PAIRED_NT[c.cin // 32] * 16
    row_blocks = -(-c.rows // rpb) * c.N
    z = 1
    while row_blocks * z < 512 and (c.cout // 32) % (z * 2) == 0:
        z *= 2
    return z


def stem_blocks(c: Case) -> tuple:
    """(blocks launched, trips of the busiest lane through the grid-stride loop)"""
    work = c.N * c.rows * (c.cout // 8)
    blocks = min(-(-work // 256), STEM_MAX_BLOCKS)
    return blocks, -(-work // (blocks * 256))


def expected_instance(c: Case, *, thin: int = 1, w_paired: int | None = None) -> str:
    """the kernel instance pytc_pw_conv_fwd launches for the case (thin: the pw_thin knob; w_paired: the weight image handed in)"""
    wp = c.w_paired if w_paired is None else w_paired
    ti, tw, to = c.dt
    plain = c.plain and not wp and thin != 0
    if plain and c.cin == 1 and c.cout % 8 == 0 and 256 % (c.cout // 8) == 0 and tw == "bf16" and to == "bf16":
        return f"pw_stem_kernel<{ti}>"
    if plain and c.cout == 1 and ti == "bf16" and tw == "bf16" and 8 <= c.cin <= 512 and c.cin & (c.cin - 1) == 0:
        return f"pw_head_kernel<{to}>"
    if wp == 2:
        assert rowmajor_supported(c)
        big = -(-c.N * c.rows // 128) * (c.cout // GEMM_BN) >= 512
        return f"pw_gemm_lds_kernel<false, {128 if big else 64}, {32 if c.cin <= 512 else GEMM_KS}, true>"
    if wp == 1:
        assert paired_supported(c)
        ks = c.cin // 32
        return f"pw_fast_kernel<{ks}, {PAIRED_NT[ks]}> z{paired_zsplit(c)}"
    assert c.dt in GENERIC_ROUTES, c.dt
    mtt = (c.cout + 15) // 16
    return f"pw_conv_kernel<{ti}, {tw}, {to}, {4 if mtt >= 4 else (2 if mtt >= 2 else 1)}, 4>"


GENERIC_ROUTES = (("f32", "f32", "f32"), ("bf16", "bf16", "bf16"), ("bf16", "bf16", "f32"), ("f32", "bf16", "bf16"))
B3 = ("bf16", "bf16", "bf16")
GENERIC_ROWS = (1, 15, 17, 255, 257)


def _generic_cases() -> list:
    out = []
    variants = (dict(), dict(ab=True), dict(res="add", bias=False), dict(ab=True, res="add"), dict(act="gelu", res="add"), dict(pre_gelu=True),
                dict(ab=True, pre_gelu=True, bias=False))
    for i, rt in enumerate(GENERIC_ROUTES):
        tails = (13, 20, 1, 32, 4) if rt[1] == "f32" else (13, 24, 48, 1, 64)
        for j, cout in enumerate((3, 12, 13, 40, 80)):
            for q in range(2):
                cin = tails[(i + j + 2 * q) % 5]
                rows = GENERIC_ROWS[(2 * i + j + 3 * q) % 5]
                var = dict(variants[(i + 2 * j + 3 * q) % 7])
                if var.get("act") == "gelu" and rows == 1:
                    rows = 17                                           # a store that rounds needs more than a handful of outputs
                if cin == 1 and not (var.get("ab") or var.get("res") or var.get("pre_gelu")):
                    var["ab"] = True                                    # C_in = 1 on a non-plain call: stays on the MFMA kernel
                tag = "-".join(k if v is True else f"{k}_{v}" for k, v in var.items() if v is not False) or "plain"
                out.append(Case("generic", f"{'_'.join(rt)}-{cin}-{cout}-{tag}-r{rows}", rt, cin, cout, 3, rows, **var,
                                edge=f"K tail {cin}, channel tail {cout}, {rows} rows"))
    for rt in (B3, GENERIC_ROUTES[0], GENERIC_ROUTES[3]):
        for g in ((5, 6, 7), (1, 1, 1), (2, 1, 3)):
            rows = int(np.prod([(v + 1) // 2 for v in g]))
            out.append(Case("generic", f"{'_'.join(rt)}-24-13-gather{'x'.join(map(str, g))}", rt, 24, 13, 3, rows, ab=g != (1, 1, 1), gather=g,
                            edge="stride-2 gather"))
    for rt, cout in ((B3, 12), (GENERIC_ROUTES[0], 13), (GENERIC_ROUTES[2], 40)):
        for res, rb in (("up_low", True), ("up_low", False), ("up", True), ("up", False)):
            out.append(Case("generic", f"{'_'.join(rt)}-24-{cout}-{res}-{'bias' if rb else 'nobias'}", rt, 24, cout, 3, 48, res=res, res_bias=rb,
                            grid=(2, 4, 6), edge="RES_UPSAMPLE, front faces = the skip alone"))
    out.append(Case("generic", "bf16-48-13-gelu_bwd", B3, 48, 13, 3, 17, bias=False, res="gelu_bwd", edge="RES_GELU_BWD on the guarded store"))
    out.append(Case("generic", "f32-20-12-gelu_bwd", GENERIC_ROUTES[0], 20, 12, 3, 17, bias=False, res="gelu_bwd", edge="RES_GELU_BWD in fp32"))
    return out


def _thin_cases() -> list:
    out = []
    for ti in ("f32", "bf16"):
        rt = (ti, "bf16", "bf16")
        out.append(Case("stem", f"{ti}-8-r257", rt, 1, 8, 3, 257, edge="one chunk, rows no multiple of 256"))
        out.append(Case("stem", f"{ti}-32-r301", rt, 1, 32, 3, 301, bias=ti == "bf16", edge="four chunks, rows no multiple of 64"))
        out.append(Case("stem", f"{ti}-256-r37", rt, 1, 256, 2, 37, edge="32 chunks, rows no multiple of 8"))
        out.append(Case("stem", f"{ti}-24-generic", rt, 1, 24, 3, 257, edge="256 % 3 != 0: the generic kernel"))
    out.append(Case("stem", "f32-256-above-cap", ("f32", "bf16", "bf16"), 1, 256, 2, 32800, edge="2 099 200 lanes of work: a second grid-stride trip"))
    out.append(Case("stem", "bf16-256-at-cap", ("bf16", "bf16", "bf16"), 1, 256, 2, 32768, edge="2 097 152 lanes of work: 8192 blocks, one trip"))
    for to in ("bf16", "f32"):
        rt = ("bf16", "bf16", to)
        # one output each: the draws (seed) are those at which that output's store rounds up and no k step's products cancel
        out.append(Case("head", f"{to}-8-r1", rt, 8, 1, 1, 1, seed=2 if to == "bf16" else 0, edge="one chunk, no shuffle, one row"))
        out.append(Case("head", f"{to}-64-r7", rt, 64, 1, 1, 7, bias=to == "f32", edge="eight chunks, seven rows"))
        out.append(Case("head", f"{to}-512-r513", rt, 512, 1, 3, 171, edge="a whole wave per row, 513 rows"))
        out.append(Case("head", f"{to}-512-r1", rt, 512, 1, 1, 1, seed=1 if to == "f32" else 0, edge="a whole wave per row, one row"))
        out.append(Case("head", f"{to}-24-generic", rt, 24, 1, 3, 171, edge="C_in no power of two: the generic kernel"))
        out.append(Case("head", f"{to}-1024-generic", rt, 1024, 1, 3, 171, edge="C_in above 512: the generic kernel"))
    return out


def _paired_cases() -> list:
    out = []
    couts = (32, 96, 192, 256, 64, 32)
    for i, cin in enumerate((32, 64, 128, 256, 512, 1024)):
        nt = PAIRED_NT[cin // 32]
        tail = 4 * nt * 16 + 5           # a second workgroup whose wave 0 holds five rows and whose waves 1-3 hold none
        out.append(Case("paired", f"{cin}-{couts[i]}-ab-add-r{tail}", B3, cin, couts[i], 3, tail, ab=True, res="add",
                        edge="partial tile + idle waves (the early return behind the L2 warm-up)"))
        out.append(Case("paired", f"{cin}-{couts[(i + 2) % 6]}-pregelu-nobias-r1", B3, cin, couts[(i + 2) % 6], 2, 1, bias=False, pre_gelu=True,
                        edge="one row: every lane reads the clamped row"))
    out.append(Case("paired", "32-256-z8", B3, 32, 256, 1, 37, edge="eight pairs over eight z shares"))
    out.append(Case("paired", "64-192-z2", B3, 64, 192, 2, 100, bias=False, edge="six pairs: two shares at most"))
    out.append(Case("paired", "128-96-z1", B3, 128, 96, 2, 70, edge="three pairs: no split possible"))
    out.append(Case("paired", "32-64-512-row-blocks", B3, 32, 64, 2, 65300, res="add", edge="512 row blocks: the split stays 1"))
    out.append(Case("paired", "32-64-gather-ab", B3, 32, 64, 3, 3 * 3 * 4, ab=True, gather=(5, 6, 7), edge="gather on an odd grid"))
    out.append(Case("paired", "256-128-gather", B3, 256, 128, 2, 3 * 3 * 4, gather=(5, 6, 7), bias=False, edge="gather on an odd grid, KS 8"))
    out.append(Case("paired", "128-64-gelu_bwd", B3, 128, 64, 3, 133, bias=False, res="gelu_bwd", edge="RES_GELU_BWD"))
    out.append(Case("paired", "1024-32-gelu_bwd", B3, 1024, 32, 2, 69, bias=False, res="gelu_bwd", edge="RES_GELU_BWD, KS 32"))
    out.append(Case("paired", "256-96-norm_bwd", B3, 256, 96, 3, 133, bias=False, res="norm_bwd", edge="RES_NORM_BWD, per-sample coefficients"))
    out.append(Case("paired", "64-32-norm_bwd-ab", B3, 64, 32, 3, 261, ab=True, res="norm_bwd", edge="RES_NORM_BWD with affine and bias"))
    out.append(Case("paired", "64-32-norm_bwd_crop", B3, 64, 32, 2, 60, bias=False, res="norm_bwd_crop", grid=(3, 4, 5), edge="cropped RES_NORM_BWD"))
    out.append(Case("paired", "512-256-norm_bwd_crop", B3, 512, 256, 3, 90, bias=False, res="norm_bwd_crop", grid=(2, 5, 9), edge="cropped RES_NORM_BWD, KS 16"))
    for i, (res, rb) in enumerate((("up_low", True), ("up_low", False), ("up", True), ("up", False))):
        cin = (32, 128, 64, 512)[i]
        out.append(Case("paired", f"{cin}-{(32, 64)[i % 2]}-{res}-{'bias' if rb else 'nobias'}", B3, cin, (32, 64)[i % 2], 3, 48, ab=i == 0, res=res,
                        res_bias=rb, grid=(2, 4, 6), edge="RES_UPSAMPLE"))
    return out


def _rowmajor_cases() -> list:
    small = dict(dt=B3, cin=64, cout=128, N=3, rows=100)       # 300 rows: 64-row tiles 1, 3 and 4 straddle a sample boundary
    out = [Case("rowmajor", "64-128-ab-norm_bwd", ab=True, res="norm_bwd", edge="64-row tiles across samples, per-sample ab and coefficients", **small),
           Case("rowmajor", "64-128-pregelu-nobias", bias=False, pre_gelu=True, edge="pre_gelu", **small),
           Case("rowmajor", "64-128-ab-pregelu-add", ab=True, pre_gelu=True, res="add", edge="affine then pre_gelu, RES_ADD", **small),
           Case("rowmajor", "64-128-gelu_bwd", bias=False, res="gelu_bwd", edge="RES_GELU_BWD", **small),
           Case("rowmajor", "64-128-norm_bwd_crop", bias=False, res="norm_bwd_crop", grid=(4, 5, 5), edge="cropped RES_NORM_BWD", **small),
           Case("rowmajor", "64-128-up_low", B3, 64, 128, 3, 48, ab=True, res="up_low", grid=(2, 4, 6), edge="RES_UPSAMPLE with res_low"),
           Case("rowmajor", "64-128-up-nobias", B3, 64, 128, 3, 48, res="up", res_bias=False, grid=(2, 4, 6), edge="RES_UPSAMPLE, holes = 0"),
           Case("rowmajor", "576-128-ab-add", B3, 576, 128, 3, 100, ab=True, res="add", edge="the wide-k instance in 64-row tiles"),
           Case("rowmajor", "64-1024-r8064-ab-add", B3, 64, 1024, 4, 2016, ab=True, res="add", edge="504 tiles of 128 rows: still the 64-row kernel"),
           Case("rowmajor", "64-1024-r8065-ab-norm_bwd", B3, 64, 1024, 5, 1613, ab=True, bias=False, res="norm_bwd",
                edge="512 tiles: the 128-row kernel, tiles across samples"),
           Case("rowmajor", "576-1024-r8065-ab-add", B3, 576, 1024, 5, 1613, ab=True, res="add", edge="the wide-k instance in 128-row tiles")]
    return out


@lru_cache(maxsize=None)
def all_cases() -> tuple:
    out = _generic_cases() + _thin_cases() + _paired_cases() + _rowmajor_cases()
    assert len({c.id for c in out}) == len(out), "duplicate case ids"
    return tuple(out)


def cases(form: str) -> list:
    return [c for c in all_cases() if c.form == form]


def ids(cs) -> list:
    return [c.id for c in cs]


# ------------------------------------------------------------------------------------------------------------- operands
def _pick(rng, values, shape):
    return np.asarray(values, dtype=np.float64)[rng.integers(0, len(values), size=shape)]


def gather_src(grid: tuple) -> np.ndarray:
    """input row of every output row of the stride-2 gather"""
    D, H, W = grid
    z, y, x = np.meshgrid(np.arange(0, D, 2), np.arange(0, H, 2), np.arange(0, W, 2), indexing="ij")
    return ((z * H + y) * W + x).reshape(-1)


def upsample_parts(grid: tuple):
    """RES_UPSAMPLE: (face mask, res_low-position mask, index into res_low rows) per output row"""
    D, H, W = grid
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    face = (z == 0) | (y == 0) | (x == 0)
    oz, oy, ox = z - 1, y - 1, x - 1
    even = ~face & (((oz | oy | ox) & 1) == 0)
    low = ((oz >> 1) * (H // 2) + (oy >> 1)) * (W // 2) + (ox >> 1)
    return face.reshape(-1), even.reshape(-1), np.where(even, low, 0).reshape(-1)


def crop_rows(grid: tuple) -> np.ndarray:
    """cropped RES_NORM_BWD: the padded-grid rows that are stored, in the order of the compact grid"""
    D, H, W = grid
    z, y, x = np.meshgrid(np.arange(1, D), np.arange(1, H), np.arange(1, W), indexing="ij")
    return ((z * H + y) * W + x).reshape(-1)


@lru_cache(maxsize=2)
def _operands(key: tuple) -> dict:
    c = _key_case(key)
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    N, R, Rin, cin, cout = c.N, c.rows, c.rows_in, c.cin, c.cout
    ti, tw, to = c.dt
    fam = family(c)
    g = np.arange(N * Rin).reshape(N, Rin)
    d = {"family": fam}
    # ---- the effective input (before the operand conversion) and the weight
    if fam == "onehot":
        xe = np.zeros((N, Rin, cin))
        np.put_along_axis(xe, (g % cin)[..., None], 1.0, 2)
        bias = _pick(rng, (0.0, 16.0), cout)
        w = np.where(bias[:, None] == 0, 16.0, -16.0) * rng.integers(0, 2, (cout, cin))
    else:
        if fam == "sparse":
            xe = np.zeros((N, Rin, cin))
            np.put_along_axis(xe, ((2 * g) % cin)[..., None], _pick(rng, (1.0, -1.0), (N, Rin, 1)), 2)
            np.put_along_axis(xe, ((2 * g + 1) % cin)[..., None], _pick(rng, (1.0, -1.0), (N, Rin, 1)), 2)
        elif fam == "dense":
            xe = _pick(rng, (1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 0.0)[:9 if N * Rin >= 8 else 8], (N, Rin, cin))
        else:
            xe = _pick(rng, (1.0, -1.0), (N, Rin, cin))
        fine = 1.0 + 2.0 ** -9 if tw == "f32" else 1.0 + 3.0 / 128
        wv = (0.5, -0.5, 1.0, -1.0, fine, -fine)
        if fam == "dense":
            w = np.zeros((cout, cin))
            o = np.arange(cout)
            w[o, (2 * o) % cin] = _pick(rng, wv, cout)
            if cin > 1:
                w[o, (2 * o + 1) % cin] = _pick(rng, wv, cout)
        else:
            w = _pick(rng, wv, (cout, cin))
        if c.pre_gelu:
            xe, w = 16.0 * np.abs(xe), w / 16.0
        elif ti == "f32" and tw == "f32":
            xe = xe * (1.0 + 2.0 ** -9)
        elif ti == "f32":
            xe = xe * (1.0 + _pick(rng, (3.0, 4.0, 5.0, 12.0), xe.shape) * 2.0 ** -10)
        bias = _pick(rng, (-0.75, -0.25, 0.25, 0.75, 1.25), cout) + _pick(rng, (1.0, 3.0, 5.0, 7.0), cout) * 2.0 ** -9
    d["w"] = w + 0.0
    d["bias"] = bias if c.bias or fam == "onehot" else None
    if c.act == "gelu" and not c.bias:
        raise AssertionError("act = GELU cases carry their bias")
    # ---- the stored input and the affine
    if c.ab:
        a = _pick(rng, (0.5, 1.0, 2.0), (N, cin))
        b0 = _pick(rng, (-1.0, -0.5, 0.0, 0.5, 1.0), (N, cin))
        t = (xe - b0[:, None, :]) / a[:, None, :]
        b = b0 + 0.0
        if ti == "bf16" and tw == "bf16" and not c.pre_gelu:
            delta = _pick(rng, (0.0, 3.0, 5.0), (N, cin)) * 2.0 ** -9
            b, xe = b0 + delta, xe + delta[:, None, :]
        d["ab"] = np.stack([a, b], 1)
        d["x"] = t + 0.0
    else:
        d["ab"] = None
        d["x"] = xe + 0.0
    d["xe"] = xe + 0.0
    # ---- epilogue operands, as values of the output type
    shape = (N, R, cout)
    f32_bit = 2.0 ** -12 if to == "f32" else 0.0
    if c.res == "add":
        q = 3.0 / 32 if c.act == "gelu" else 0.25
        d["res"] = rng.integers(-8, 9, shape) * q + f32_bit
    elif c.res == "gelu_bwd":
        d["res"] = _pick(rng, (0.0, 16.0, -16.0), shape)
    elif c.res in ("norm_bwd", "norm_bwd_crop"):
        d["res"] = rng.integers(-8, 9, shape) * 0.25
        d["coef"] = np.stack([_pick(rng, (0.5, 1.0, 2.0), (N, cout)), _pick(rng, (-0.5, 0.25, 0.5, 1.0), (N, cout)),
                              rng.integers(-6, 7, (N, cout)) * 0.25], 1)
    elif c.res in ("up", "up_low"):
        d["res"] = rng.integers(-8, 9, shape) * 0.25 + f32_bit
        if c.res == "up_low":
            d["res_low"] = rng.integers(-8, 9, (N, R // 8, cout)) * 0.25
        if c.res_bias:
            d["res_bias"] = rng.integers(-6, 7, cout) * 0.25 + 0.125
    return d


def operands(c: Case) -> dict:
    """float64 numpy operands of a case (treat as read-only): x (the STORED input, [N][rows_in][C_in]), ab, w [C_out][C_in], bias, res ..."""
    return _operands(c.data_key)


def is_f32(v: np.ndarray) -> bool:
    return bool((np.asarray(v, np.float64).astype(np.float32).astype(np.float64) == v).all())


def bf16_trunc_np(v: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 by dropping the low 16 bits: the conversion the kernels must NOT use"""
    b = np.ascontiguousarray(np.asarray(v, np.float64).astype(np.float32)).view(np.uint32) & np.uint32(0xFFFF0000)
    return b.view(np.float32).astype(np.float64)


def _f32_image(v: np.ndarray) -> np.ndarray:
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def _gelu_loose(v: np.ndarray) -> np.ndarray:
    """a MUTATED reference may leave the exact points: the erf GELU in fp64, as an fp32 number (it only has to differ)"""
    return _f32_image(torch.nn.functional.gelu(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))).numpy())


def operand_values(c: Case, d: dict, x: np.ndarray, n_idx, *, trunc: bool = False, strict: bool = True) -> np.ndarray:
    """the MFMA B operand of input rows x (M, C_in) that belong to samples n_idx (M,): affine, pre_act, conversion.  strict = False
    (the mutated references of `discrimination`): values need not be exact, they are rounded to fp32 where the kernel would round"""
    ab = d["ab"]
    v = x
    if c.ab:
        v = x * ab[n_idx, 0] + ab[n_idx, 1]
        assert not strict or is_f32(v), "fmaf(t, a, b) must be exact in fp32"
        v = _f32_image(v)
    if c.pre_gelu:
        assert not strict or np.isin(v, GELU_EXACT_VALUES).all(), "pre_act = GELU away from its exact points"
        if not strict:
            v = _gelu_loose(v)
    if c.dt[1] == "bf16":
        v = bf16_trunc_np(v) if trunc else bf16_np(v)
    return v


def finish(c: Case, d: dict, acc: np.ndarray, n_idx, r_idx, *, coef=None, low_shift: int = 0, strict: bool = True) -> np.ndarray:
    """the epilogue in fp64 on the GEMM sums acc (M, C_out) of output rows (n_idx, r_idx) -> the unrounded outputs"""
    v = acc + 0.0
    if d["bias"] is not None:
        v = v + d["bias"]
    if c.act == "gelu":
        assert not strict or np.isin(v, GELU_EXACT_VALUES).all(), "act = GELU away from its exact points"
        if not strict:
            v = _gelu_loose(v)
    if c.res == "none":
        return v
    res = d["res"][n_idx, r_idx]
    if c.res == "add":
        return v + res
    if c.res == "gelu_bwd":
        grad = np.select([res == k for k in GELU_GRAD_EXACT], list(GELU_GRAD_EXACT.values()), np.nan)
        assert not np.isnan(grad).any()
        return v * grad
    if c.res in ("norm_bwd", "norm_bwd_crop"):
        cf = d["coef"] if coef is None else coef
        return cf[n_idx, 0] * v + (cf[n_idx, 1] * res + cf[n_idx, 2])
    face, even, low = upsample_parts(c.grid)
    rl = np.zeros_like(v) + (d["res_bias"] if c.res_bias else 0.0)
    if c.res == "up_low":
        e = even[r_idx]
        nlow = d["res_low"].shape[1]
        rl[e] = d["res_low"][n_idx[e], (low[r_idx[e]] + low_shift) % nlow]
    return np.where(face[r_idx][:, None], res, v + rl + res)


def to_out(c: Case, v: np.ndarray, *, trunc: bool = False, strict: bool = True) -> torch.Tensor:
    """one rounding into the output type"""
    assert not strict or is_f32(v), "an output is not an fp32 number: the premise does not hold"
    v = _f32_image(v)
    if c.dt[2] == "f32":
        return torch.from_numpy(v.astype(np.float32))
    if trunc:
        b = np.ascontiguousarray(v.astype(np.float32)).view(np.uint32) >> np.uint32(16)
        return torch.from_numpy(b.astype(np.uint16).view(np.int16)).view(torch.bfloat16)
    return to_bf16(v)


def out_bits(c: Case, v: np.ndarray, **kw) -> np.ndarray:
    t = to_out(c, v, **kw)
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).numpy()


def all_rows(c: Case):
    n = np.repeat(np.arange(c.N), c.rows)
    return n, np.tile(np.arange(c.rows), c.N)


def src_rows(c: Case, r_idx, shift: tuple = (0, 0, 0)):
    """input row of output rows r_idx (the gather, optionally displaced by `shift` voxels, wrapping inside the grid)"""
    if not c.gather:
        return r_idx
    D, H, W = c.gather
    s = gather_src(c.gather)[r_idx]
    z, y, x = s // (H * W), s // W % H, s % W
    return (((z + shift[0]) % D) * H + (y + shift[1]) % H) * W + (x + shift[2]) % W


@lru_cache(maxsize=2)
def _reference(key: tuple) -> dict:
    c = _key_case(key)
    d = _operands(key)
    n, r = all_rows(c)
    xq = operand_values(c, d, d["x"][n, src_rows(c, r)], n)
    acc = xq @ d["w"].T
    y64 = finish(c, d, acc, n, r).reshape(c.N, c.rows, c.cout)
    stored = y64[:, crop_rows(c.grid)] if c.res == "norm_bwd_crop" else y64
    return {"xq": xq.reshape(c.N, c.rows, c.cin), "acc": acc.reshape(c.N, c.rows, c.cout), "y64": y64, "y": to_out(c, stored)}


def reference(c: Case) -> dict:
    """xq (the MFMA operand), acc (the GEMM sums), y64 (unrounded, every row) and y (the stored tensor in the output type)"""
    return _reference(c.data_key)


# ------------------------------------------------------------------------------------------------------------- premises
def unit_exp(*arrs) -> int:
    """the largest e with every entry of every array a multiple of 2^e"""
    e = 1 << 20
    for a in arrs:
        for v in np.unique(np.abs(np.asarray(a, np.float64))):
            if v == 0:
                continue
            p, q = float(v).as_integer_ratio()
            e = min(e, (p & -p).bit_length() - 1 if q == 1 else -(q.bit_length() - 1))
    return e


def assert_premises(c: Case) -> dict:
    """every output's terms are multiples of one unit, sum |terms| < 2^24 units; stored operands are numbers of their types -> reference"""
    return _assert_premises(c.data_key)


@lru_cache(maxsize=2)
def _assert_premises(key: tuple) -> dict:
    c = _key_case(key)
    d, ref = _operands(key), _reference(key)
    ti, tw, to = c.dt
    for name, t in (("x", ti), ("w", tw), ("res", to), ("res_low", to)):
        if d.get(name) is not None:
            assert (bf16_np(d[name]) == d[name]).all() if t == "bf16" else is_f32(d[name]), f"{c.id}: {name} is not a {t} tensor"
    for name in ("bias", "ab", "coef", "res_bias"):
        assert d.get(name) is None or is_f32(d[name]), f"{c.id}: {name} is not fp32"
    if ti == "f32" and not c.pre_gelu and c.act != "gelu":
        nzx = d["xe"][d["xe"] != 0]
        assert (bf16_np(nzx) != nzx).all(), f"{c.id}: fp32 inputs must lie off the bf16 grid"
        if tw == "bf16":
            assert (bf16_trunc_np(nzx) != bf16_np(nzx)).any()
    if tw == "f32" and c.act != "gelu":
        assert (bf16_np(d["w"]) != d["w"]).any(), f"{c.id}: fp32 weights must not all be bf16 numbers"
    if c.res == "gelu_bwd":
        assert {float(v) for v in np.unique(d["res"])} == set(GELU_GRAD_EXACT), c.id
    xq, w = ref["xq"], d["w"]
    scale = np.ones((c.N, 1, c.cout))                       # what multiplies the GEMM sum in the epilogue
    units = [unit_exp(xq) + unit_exp(w)]
    total = np.abs(xq) @ np.abs(w).T
    if d["bias"] is not None:
        units.append(unit_exp(d["bias"]))
        total = total + np.abs(d["bias"])
    extra = 0.0
    if c.res == "add":
        units.append(unit_exp(d["res"]))
        extra = np.abs(d["res"])
    elif c.res == "gelu_bwd":
        units = [u - 1 for u in units]                     # the factor 1/2
    elif c.res in ("norm_bwd", "norm_bwd_crop"):
        cf = d["coef"]
        scale = np.abs(cf[:, 0])[:, None, :]
        units = [u + unit_exp(cf[:, 0]) for u in units] + [unit_exp(cf[:, 1]) + unit_exp(d["res"]), unit_exp(cf[:, 2])]
        extra = np.abs(cf[:, 1])[:, None, :] * np.abs(d["res"]) + np.abs(cf[:, 2])[:, None, :]
    elif c.res in ("up", "up_low"):
        units.append(unit_exp(d["res"]))
        extra = np.abs(d["res"])
        for k in ("res_low", "res_bias"):
            if d.get(k) is not None:
                units.append(unit_exp(d[k]))
                extra = extra + np.abs(d[k]).max()
    u = min(units)
    worst = float((total * scale + extra).max()) * 2.0 ** -u
    assert worst < 2.0 ** EXACT_BITS, f"{c.id}: sum |terms| reaches {worst:.0f} units of 2^{u}: not below 2^24"
    out = dict(ref)
    out["unit_exp"], out["worst_units"] = u, worst
    return out


# ------------------------------------------------------------------------------------------------------------- discrimination
def witness_rows(c: Case, limit: int = 1024):
    """(n, r) of the rows the mutation checks look at: all of them, or the first and last `limit` global rows"""
    n, r = all_rows(c)
    if len(n) > 2 * limit:
        keep = np.r_[0:limit, len(n) - limit:len(n)]
        n, r = n[keep], r[keep]
    return n, r


def kstep_widths(c: Case) -> tuple:
    if c.form == "rowmajor":
        return (32, GEMM_KS)
    return (KSTEP[c.dt[1]],)


def applicable(c: Case) -> dict:
    """which mutations can show in a case at all (the others have nothing to act on)"""
    return {
        "kstep": True, "channel": True, "transpose": c.cin > 1 and c.cout > 1,       # one row or one column: the same memory either way
        "ab0": c.ab, "coef0": c.res in ("norm_bwd", "norm_bwd_crop"),
        "gather_shift": bool(c.gather) and max(c.gather) > 1,
        "low_shift": c.res == "up_low",
        # a lone product of the filed operands (the stem without bias) never lies past a midpoint of the bf16 grid
        "trunc_store": c.dt[2] == "bf16" and not (c.cin == 1 and not c.bias and c.res == "none"),
        "trunc_operand": c.rounds_operand and not c.pre_gelu and c.act != "gelu",       # {0, 1, 16} are bf16 numbers
        "zshare": c.form == "paired" and paired_zsplit(c) > 1,
    }


def discrimination(c: Case) -> dict:
    """mutation -> number of witness outputs whose stored bits change (the host test asserts > 0 for every applicable one; for "kstep"
    and "channel" the MINIMUM over all k steps / input channels)"""
    d, ref = operands(c), reference(c)
    app = applicable(c)
    n, r = witness_rows(c)
    xq, acc = ref["xq"][n, r], ref["acc"][n, r]
    w = d["w"]
    live = np.ones(len(n), bool)
    if c.res == "norm_bwd_crop":
        live = np.isin(r, crop_rows(c.grid))
    elif c.res in ("up", "up_low"):
        live = ~upsample_parts(c.grid)[0][r]               # the front faces take the skip alone
    n, r, xq, acc = n[live], r[live], xq[live], acc[live]
    base = out_bits(c, finish(c, d, acc, n, r))

    def changed(acc2=None, **kw) -> int:
        return int((out_bits(c, finish(c, d, acc if acc2 is None else acc2, n, r, strict=False, **kw), strict=False) != base).sum())

    out = {}
    worst = None
    for width in kstep_widths(c):
        for k0 in range(0, c.cin, width):
            sl = slice(k0, min(k0 + width, c.cin))
            cnt = changed(acc - xq[:, sl] @ w[:, sl].T)
            worst = cnt if worst is None else min(worst, cnt)
    out["kstep"] = worst
    # a single input channel: two witness rows per channel
    worst = None
    full_n, full_r = all_rows(c)
    xq_all = ref["xq"].reshape(-1, c.cin)
    for k in range(c.cin):
        rows_k = np.nonzero(xq_all[:, k])[0]
        if c.res == "norm_bwd_crop":
            rows_k = rows_k[np.isin(full_r[rows_k], crop_rows(c.grid))]
        elif c.res in ("up", "up_low"):
            rows_k = rows_k[~upsample_parts(c.grid)[0][full_r[rows_k]]]
        rows_k = rows_k[np.argsort(-np.abs(xq_all[rows_k, k]), kind="stable")[:16]]     # the rows in which the channel weighs most
        if not len(rows_k):
            worst = 0
            break
        nk, rk = full_n[rows_k], full_r[rows_k]
        a0 = ref["acc"].reshape(-1, c.cout)[rows_k]
        a1 = a0 - xq_all[rows_k, k][:, None] * w[None, :, k]
        cnt = int((out_bits(c, finish(c, d, a1, nk, rk, strict=False), strict=False) != out_bits(c, finish(c, d, a0, nk, rk))).sum())
        worst = cnt if worst is None else min(worst, cnt)
    out["channel"] = worst
    if app["transpose"]:
        out["transpose"] = changed(xq @ w.reshape(-1).reshape(c.cin, c.cout))
    x_src = d["x"][n, src_rows(c, r)]
    if app["ab0"]:
        out["ab0"] = changed(operand_values(c, d, x_src, np.zeros_like(n), strict=False) @ w.T)
    if app["coef0"]:
        out["coef0"] = changed(coef=np.broadcast_to(d["coef"][:1], d["coef"].shape))
    if app["gather_shift"]:
        worst = None
        for ax in range(3):
            if c.gather[ax] > 1:
                sh = tuple(int(i == ax) for i in range(3))
                cnt = changed(operand_values(c, d, d["x"][n, src_rows(c, r, sh)], n, strict=False) @ w.T)
                worst = cnt if worst is None else min(worst, cnt)
        out["gather_shift"] = worst
    if app["low_shift"]:
        out["low_shift"] = changed(low_shift=1)
    if app["trunc_store"]:
        out["trunc_store"] = int((out_bits(c, finish(c, d, acc, n, r), trunc=True) != base).sum())
    if app["trunc_operand"]:
        out["trunc_operand"] = changed(operand_values(c, d, x_src, n, trunc=True, strict=False) @ w.T)
    if app["zshare"]:
        # a share that is skipped leaves its channels unwritten (the GPU test's NaN fill shows it); a share that computes share 0's
        # pairs instead must show too
        z = paired_zsplit(c)
        per = c.cout // z
        full = finish(c, d, acc, n, r)
        worst = None
        for s in range(1, z):
            wrong = full.copy()
            wrong[:, s * per:(s + 1) * per] = full[:, :per]
            cnt = int((out_bits(c, wrong, strict=False) != base).sum())
            worst = cnt if worst is None else min(worst, cnt)
        out["zshare"] = worst
    return out


# ------------------------------------------------------------------------------------------------------------- weight images
def packed_model(w: np.ndarray, tw: str) -> np.ndarray:
    """pytc_pw_pack_weight: element (o, k) at tile o / 16, k group k / KSTEP, lane (o % 16) + 16 ((k % KSTEP) / EPL), slot k % EPL;
    zero padding (the comment of packed_weight in csrc/pw_kernels.hip)"""
    cout, cin = w.shape
    ks, epl = KSTEP[tw], EPL[tw]
    KG, MT = -(-cin // ks), -(-cout // 16)
    img = np.zeros((MT, KG, 64, epl))
    o, k = np.meshgrid(np.arange(cout), np.arange(cin), indexing="ij")
    img[o // 16, k // ks, o % 16 + 16 * (k % ks // epl), k % epl] = w
    return img.reshape(-1)


def packed_paired_model(w: np.ndarray) -> np.ndarray:
    """pytc_pw_pack_weight_paired (bf16): the same image with row m of tile T holding output channel paired_row(T, m)"""
    cout, cin = w.shape
    assert cout % 32 == 0
    perm = np.array([paired_row(T, m) for T in range(cout // 16) for m in range(16)])
    return packed_model(w[perm], "bf16")


def packed_elems_model(cout: int, cin: int, tw: str) -> int:
    return -(-cout // 16) * 16 * -(-cin // KSTEP[tw]) * KSTEP[tw]

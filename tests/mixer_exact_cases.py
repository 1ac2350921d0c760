"""Exact-arithmetic cases for the fused channel mixers  y = W3 gelu(W2 (a t + b) + b2) + b3 (+ residual)  (CPU only, numpy + torch).

The path the models run (hip_ops.MLP_F16_PROJECT) evaluates GELU with gelu_h8_from_f32 (csrc/pytc_common.h): a FIXED chain of IEEE
fp16 operations with no transcendental in it, so a CPU model gives its bits:

  x16 = fp32 -> f16, round toward zero, saturating at +-65504      (v_cvt_pkrtz_f16_f32)
  u   = min(|x16|, 3.75)                                            exact
  t   = fma(u, f16(2 / 3.75), -1)                                   one rounding
  p   = c7;  p = fma(p, t, c_k)  for k = 6 .. 0                     one rounding each; c_k = f16(fp32 literal)
  g   = max(x16, 0) - p                                             one rounding

gelu_h8_model evaluates every FMA in float64 -- exact there: both factors are f16 numbers of magnitude <= 4 with their last bit at
2^-24 or above, so the 22-bit product has its last bit at 2^-48 or above and product + addend span fewer than 53 bits -- and rounds
ONCE to float16 (numpy's float64 -> float16 conversion is a single correctly rounded step, subnormals included).

Operands (every case; tests/test_host_mixer_exact_cases.py proves the premises case by case through assert_premises below):

  effective input  x = a t + b  (the affine form; the folded form feeds x itself as t).  Two families, so that the k loops of both GEMMs
           are exercised:  "sparse": two non-zeros +-1 per row whose positions rotate with (sample, row) -- every input channel and
           every 32-wide k step occurs -- against a DENSE W2 drawn per (j, k) from {+-1/2, +-1};  "dense": integers in [-1, 1] with few
           zeros against a W2 with two non-zeros per row from {+-1/2, +-1} (every input channel used wherever 2 C_hid >= C_in).
  affine   a in {1/2, 1, 2}, b a multiple of 1/2, per (sample, channel), different in every sample; the stored t = (x - b) / a is a
           multiple of 1/4, so fma(t, a, b) and its bf16 image are exact and the affine form is the SAME function of other operands.
  folded   per-sample images W2_n = diag(s_n) W2 and vectors b2_n (s_n = +-1 per (sample, hidden channel)): different in every sample.
  b2       odd quarters {+-1/4, +-3/4}: every pre-activation h is an ODD multiple of 1/4 with |h| <= 2.75 -- never 0 (gelu_h2(0) is
           2^-14), never in the saturated negative tail (units of 2^-23).
  W3       (f16 image) two non-zeros per hidden channel from {+-1/2, +-1, +-2}, at outputs (j mod C_out) and a second one that differs
           for every hidden channel sharing the first: every hidden channel feeds an output, no two channels share a pattern, an output
           row holds 2 C_hid / C_out terms.
  b3, residual, skip, res_low, res_bias, stem operands: quarters of magnitude <= 2 (the stem input: small integers).
  head / projection images: integers in [-2, 2]; their biases quarters.

Premise, asserted for EVERY output element of EVERY case (exact_sum below): all terms of its sum -- products, bias, residual -- are
multiples of a unit 2^-k, and sum |terms| < 2^24 * 2^-k.  Then every partial sum in ANY order is an fp32 number: both MFMA sums and the
epilogue add are exact, and the ONLY rounding of an output is its store as bf16.  The reference is the fp64 sum over the model's hidden
values, rounded once to bf16 (it fits fp32 exactly by the premise, so torch's float64 -> float32 -> bfloat16 route rounds once).

"conv" cases use b2 = 1 + k 2^-14 (k odd, 1/8 <= k 2^-14 <= 1/4): h is then neither an f16 nor a bf16 number, which pins round-toward-zero into the f16 hidden
and, in the training forward, GELU evaluated at the STORED bf16(h).

Every case also proves that its tensor discriminates: truncation of the output differs from round-to-nearest on at least
min_trunc_diff(case) outputs, and dropping ANY single 32-wide hidden chunk changes at least one output."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

BF16 = torch.bfloat16
EXACT_BITS = 24                      # fp32 significand: sums of multiples of a unit stay exact below 2^24 units

# ------------------------------------------------------------------------------------------------------------- the GELU bit model
GELU_U = 3.75
GELU_COEFFS = (-6.166994737e-02, 6.367329291e-02, 1.683184914e-01, -3.056981228e-01, 7.903670132e-02, 1.852329106e-01,
               -1.855973189e-01, 5.694380662e-02)          # c7 .. c0 of csrc/pytc_common.h


def _h(v) -> np.float64:
    """(_Float16)(float literal): fp32, then round to nearest even into f16"""
    return np.float64(np.float16(np.float32(v)))


def f32_to_f16_rtz(x: np.ndarray) -> np.ndarray:
    """v_cvt_pkrtz_f16_f32: round toward zero, finite in -> finite out (+-65504 beyond the f16 range), subnormal images kept"""
    x = np.asarray(x, dtype=np.float32)
    assert np.isfinite(x).all()
    with np.errstate(over="ignore"):
        y = x.astype(np.float16)                                        # round to nearest even
    bits = y.view(np.uint16).copy()
    inf = np.isinf(y)
    bits[inf] = (bits[inf] & 0x8000) | 0x7BFF
    away = (~inf) & (np.abs(y.astype(np.float64)) > np.abs(x.astype(np.float64)))
    bits[away] -= 1                                                     # one step toward zero (sign bit untouched: |y| > 0 here)
    return bits.view(np.float16)


def f32_to_f16_rne(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        y = np.asarray(x, dtype=np.float32).astype(np.float16)
    bits = y.view(np.uint16).copy()
    inf = np.isinf(y)
    bits[inf] = (bits[inf] & 0x8000) | 0x7BFF
    return bits.view(np.float16)


def _r16(v: np.ndarray) -> np.ndarray:
    """one rounding of an exact float64 value to f16, carried on as float64"""
    return v.astype(np.float16).astype(np.float64)


def gelu_h2_model(x16: np.ndarray, *, unfused_t: bool = False) -> np.ndarray:
    """gelu_h2 of csrc/pytc_common.h on f16 inputs -> f16.  unfused_t: t = round(round(u c) - 1), the variant the kernel must NOT be."""
    x = np.asarray(x16, dtype=np.float16).astype(np.float64)
    u = np.minimum(np.abs(x), GELU_U)
    c = _h(np.float32(2.0) / np.float32(3.75))
    t = _r16(_r16(u * c) - 1.0) if unfused_t else _r16(u * c - 1.0)
    p = np.full_like(t, _h(GELU_COEFFS[0]))
    for ck in GELU_COEFFS[1:]:
        p = _r16(p * t + _h(ck))
    return (np.maximum(x, 0.0) - p).astype(np.float16)


def gelu_h8_model(x32: np.ndarray, *, rne: bool = False, unfused_t: bool = False) -> np.ndarray:
    """gelu_h8_from_f32: fp32 array -> float16 array, the kernel's bits"""
    x16 = f32_to_f16_rne(x32) if rne else f32_to_f16_rtz(x32)
    return gelu_h2_model(x16, unfused_t=unfused_t)


def erf_gelu64(x: np.ndarray) -> np.ndarray:
    return torch.nn.functional.gelu(torch.from_numpy(np.asarray(x, dtype=np.float64))).numpy()


def all_f16_in(lo: float, hi: float) -> np.ndarray:
    """every finite f16 value in [lo, hi], -0 and subnormals included"""
    v = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16).view(np.float16)
    v = v[np.isfinite(v)]
    return v[(v >= lo) & (v <= hi)]


@lru_cache(maxsize=None)
def sweep_inputs() -> dict:
    """the fp32 inputs of the GELU sweep, by group"""
    core = all_f16_in(-8.0, 8.0).astype(np.float32)
    allf = all_f16_in(-65504.0, 65504.0)
    big16 = allf[np.abs(allf) > 8.0]
    big = np.concatenate([big16[:: max(1, len(big16) // 300)].astype(np.float32),
                          np.float32([65504.0, -65504.0, 65519.0, 65520.0, -65520.0, 1e5, -1e5, 3e38, -3e38])])
    # fp32 values f16 cannot hold: either side of the midpoint between two neighbouring f16 numbers, and the midpoint itself
    base = np.float16([0.0009765625, 0.333, 0.5, 0.999, 1.0, 1.5, 2.0, 2.75, 3.0, 3.49, 3.748, 3.75, 5.0, 1000.0]).astype(np.float64)
    nxt = np.nextafter(base.astype(np.float16), np.float16(np.inf)).astype(np.float64)
    mid = (base + nxt) / 2
    ulp = nxt - base
    pts = np.concatenate([mid, mid - ulp / 4, mid + ulp / 4, mid - ulp / 2048, mid + ulp / 2048, base + ulp / 2048, nxt - ulp / 2048])
    mids = np.concatenate([pts, -pts]).astype(np.float32)
    assert (mids.astype(np.float64) == np.concatenate([pts, -pts])).all()          # all are fp32 numbers
    # values whose f16 image is subnormal (|x| < 2^-14), f16 numbers and fp32 numbers between them; none is an fp32 denormal
    sub16 = allf[(np.abs(allf) < 2.0 ** -14) & (allf != 0)].astype(np.float32)
    sub = np.concatenate([sub16[::16], sub16[::64] * np.float32(1.0 + 2.0 ** -12), np.float32([2.0 ** -25, -2.0 ** -25, 2.0 ** -30, 3e-8])])
    return {"f16 in [-8, 8]": core, "large": big, "midpoints": mids, "subnormal images": sub}


# ------------------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    group: str                   # stream | dma | lds | chunk | gemm | dwmix | conv
    name: str
    cin: int
    chid: int
    cout: int
    N: int
    rows: int
    family: str = "sparse"       # sparse | dense
    form: str = "affine"         # affine | folded
    res: str = "none"            # none | add | up | up_low | stem
    grid: tuple = ()             # RES_UPSAMPLE: the (even) output grid, rows = its product
    n_head: int = 0              # > 0: the fused output head
    head_bias: bool = True
    proj: bool = False           # the 32 -> 32 projection in the epilogue
    conv: bool = False           # conversion case: b2 = 1 + k 2^-14
    dims: tuple = ()             # dwmix: (D, H, W) of the block input; rows = D H W, res "add" = the block's own residual x
    knobs: tuple = ()

    @property
    def id(self) -> str:
        return f"{self.group}-{self.name}"

    @property
    def data_key(self) -> tuple:
        return (self.cin, self.chid, self.cout, self.N, self.rows, self.family, self.form, self.res, self.grid, self.n_head,
                self.head_bias, self.proj, self.conv, self.dims)


# (C_in / 32, C_out / 16) -> voxel tiles per wave: dispatch_mlp of csrc/pw_mlp_kernels.hip
MLP_INSTANCES = {(1, 2): 4, (1, 4): 4, (2, 2): 4, (2, 4): 2, (2, 8): 2, (4, 4): 2, (4, 8): 2, (4, 16): 1, (8, 8): 2, (8, 16): 1,
                 (8, 32): 1, (16, 16): 1, (16, 32): 1}
KNOB_DEFAULTS = {"mlp_dma": 1, "mlp_dma_rows": 1 << 20, "mlp_dma_wgs": 0, "mlp_lds_variant": 0, "mlp_chunk_variant": 0, "pw_gemm_rows": 0,
                 "dwconv_mfma": 1, "dwconv_mfma_variant": 0}
UP_GRIDS = ((2, 2, 2), (4, 4, 6), (6, 6, 8), (2, 6, 22))        # 8, 96 (tiles straddle y and z carries), 288, 264 rows


def widest_hidden(ks: int, mo: int) -> int:
    """the widest hidden layer an instance is used with: 256 -> 2048 -> 128 (expansion 8), else expansion 4, 1024 at most"""
    return 2048 if (ks, mo) == (8, 8) else min(4 * ks * 32, 1024)


def _stream_cases() -> list:
    out = []
    combos = [(f, r) for f in ("affine", "folded") for r in ("none", "add", "up", "up_low")]
    for i, ((ks, mo), nt) in enumerate(MLP_INSTANCES.items()):
        wg = 4 * nt * 16
        # 1 row (every lane reads the clamped row rps - 1), exactly one workgroup, that + 1, a tail in which whole waves have no rows
        row_choices = (1, wg, wg + 1, wg + nt * 16 + 3)
        hid_choices = (32, 64, 96, widest_hidden(ks, mo))
        q = 0
        for j, (form, res) in enumerate(combos):
            chid = hid_choices[(i + j) % 4]
            N = 3 if (i + j) % 2 else 1
            if res in ("up", "up_low"):
                grid = UP_GRIDS[(i + j // 2) % 4]
                rows = grid[0] * grid[1] * grid[2]
            else:
                grid, rows = (), row_choices[(i + q) % 4]
                q += 1
            fam = "dense" if (i + j // 4) % 2 else "sparse"
            out.append(Case("stream", f"{ks * 32}-{chid}-{mo * 16}-{form}-{res}-r{rows}-n{N}", ks * 32, chid, mo * 16, N, rows, fam, form,
                            res, grid))
    # every instance meets its widest hidden layer, all four row classes and both families at least once
    for i, ((ks, mo), nt) in enumerate(MLP_INSTANCES.items()):
        wg = 4 * nt * 16
        rows = (wg + nt * 16 + 3, 1, wg + 1, wg)[i % 4]
        out.append(Case("stream", f"{ks * 32}-{widest_hidden(ks, mo)}-{mo * 16}-wide-r{rows}", ks * 32, widest_hidden(ks, mo), mo * 16,
                        3 if i % 2 else 1, rows, "dense" if i % 2 else "sparse", "folded" if i % 2 else "affine", "add"))
    # the fused head and the stem residual on the one-tile-per-wave kernel (affine operands never take the DMA form)
    for cin, nh, hb, res in ((32, 3, True, "add"), (64, 16, False, "none"), (64, 1, True, "add")):
        out.append(Case("stream", f"head-{cin}-{nh}-{res}", cin, 64, 32, 2, 321, "dense", "affine", res, n_head=nh, head_bias=hb))
    out.append(Case("stream", "stemres-affine", 32, 64, 32, 2, 321, "sparse", "affine", "stem"))
    return out


def _dma_cases() -> list:
    """pw_mlp_dma_kernel and, with mlp_dma = 0, the HEAD / STEMRES instances of pw_mlp_kernel on folded operands.  577 rows = 10 tiles:
    with one workgroup per sample (mlp_dma_wgs = 1) waves 0 and 1 walk three tiles"""
    out = []
    shapes = ((1, 64, 1, "sparse"), (63, 96, 2, "dense"), (577, 128, 3, "sparse"), (577, 64, 2, "dense"))
    heads = ((1, True), (3, False), (16, True), (3, True))
    for (rows, chid, N, fam), (nh, hb) in zip(shapes, heads):
        for dma, wgs in ((0, 0), (1, 0), (1, 1), (1, 3)):
            kn = (("mlp_dma_rows", 0), ("mlp_dma", dma), ("mlp_dma_wgs", wgs))
            tag = f"{chid}-r{rows}-n{N}-dma{dma}-wgs{wgs}"
            for res in ("none", "add", "stem"):
                out.append(Case("dma", f"{res}-{tag}", 32, chid, 32, N, rows, fam, "folded", res, knobs=kn))
            for res in ("none", "add"):
                out.append(Case("dma", f"head{nh}-{res}-{tag}", 32, chid, 32, N, rows, fam, "folded", res, n_head=nh, head_bias=hb, knobs=kn))
                out.append(Case("dma", f"proj-{res}-{tag}", 32, chid, 32, N, rows, fam, "folded", res, proj=True, knobs=kn))
    return out


LDS_FAMILIES = ((64, 32), (64, 64), (128, 64), (128, 128))
CHUNK_FAMILIES = ((64, 32), (64, 64), (64, 128), (128, 64), (128, 128), (256, 128))


def _lds_chunk_cases() -> list:
    out = []
    for i, (cin, cout) in enumerate(LDS_FAMILIES):
        for variant in (0, 2):                      # 2: sixteen waves, the most
            # N = 3 with two tiles per sample: one workgroup's share of the (sample, tile) sequence crosses both sample boundaries
            out.append(Case("lds", f"{cin}-{2 * cin}-{cout}-affine-v{variant}", cin, 2 * cin, cout, 3, 40, "sparse", "affine",
                            ("add", "up_low", "none", "up")[i], (2, 2, 10) if i % 2 else (), knobs=(("mlp_lds_variant", variant),)))
            out.append(Case("lds", f"{cin}-{2 * cin}-{cout}-folded-v{variant}", cin, 2 * cin, cout, 3, 333, "dense", "folded",
                            ("none", "add", "add", "none")[i], knobs=(("mlp_lds_variant", variant),)))
    for i, (cin, cout) in enumerate(CHUNK_FAMILIES):
        for variant in (0, 4):                      # 4: sixteen waves, the most
            chid = (64, 96, 4 * cin)[i % 3]         # two / three chunks (ring start-up and drain; one chunk is not a shape of this kernel), wide
            out.append(Case("chunk", f"{cin}-{chid}-{cout}-affine-v{variant}", cin, chid, cout, 2, 96, "dense", "affine",
                            ("up_low", "add", "none")[i % 3], (4, 4, 6) if i % 3 == 0 else (), knobs=(("mlp_chunk_variant", variant),)))
            chid = 2048 if cin == 256 else (96, 4 * cin, 64)[i % 3]
            out.append(Case("chunk", f"{cin}-{chid}-{cout}-folded-v{variant}", cin, chid, cout, 3, 205, "sparse", "folded",
                            ("add", "none", "add")[i % 3], knobs=(("mlp_chunk_variant", variant),)))
    return out


def _gemm_cases() -> list:
    out = []
    for rk in (0, 64, 128):
        kn = (("pw_gemm_rows", rk),)
        out.append(Case("gemm", f"128-256-128-add-rows{rk}", 128, 256, 128, 3, 333, "sparse", "affine", "add", knobs=kn))
        out.append(Case("gemm", f"256-512-256-none-rows{rk}", 256, 512, 256, 1, 17, "dense", "affine", "none", knobs=kn))
        out.append(Case("gemm", f"128-256-128-up-rows{rk}", 128, 256, 128, 2, 96, "dense", "affine", "up", (4, 4, 6), knobs=kn))
        out.append(Case("gemm", f"128-512-128-uplow-rows{rk}", 128, 512, 128, 2, 264, "sparse", "affine", "up_low", (2, 6, 22), knobs=kn))
    return out


def _conv_cases() -> list:
    return [Case("conv", "32-64-32-affine", 32, 64, 32, 2, 130, "sparse", "affine", "add", conv=True),
            Case("conv", "64-64-64-affine", 64, 64, 64, 1, 97, "dense", "affine", "none", conv=True),
            Case("conv", "32-64-32-folded", 32, 64, 32, 3, 130, "dense", "folded", "add", conv=True),
            Case("conv", "128-96-128-folded", 128, 96, 128, 2, 65, "sparse", "folded", "none", conv=True)]


def _dwmix_cases() -> list:
    """the fused block: depthwise 3x3x3 conv re-formed in LDS -> folded mixer -> + x.  (8, 8, 8) and (11, 9, 12): the small-plane form
    (hi + lo weight halves always), ragged footprints, two z-chunks; (9, 16, 17): the z-march form under both weight variants"""
    def mk(name, dims, N, chid, res, variant, **kw):
        return Case("dwmix", name, 32, chid, 32, N, dims[0] * dims[1] * dims[2], "dense", "folded", res, dims=dims,
                    knobs=(("dwconv_mfma_variant", variant),), **kw)
    return [mk("8x8x8-64-res", (8, 8, 8), 3, 64, "add", 0), mk("11x9x12-96-nores", (11, 9, 12), 1, 96, "none", 0),
            mk("9x16x17-128-res-v0", (9, 16, 17), 2, 128, "add", 0), mk("9x16x17-128-res-v1", (9, 16, 17), 2, 128, "add", 1),
            mk("8x8x9-64-head3", (8, 8, 9), 2, 64, "add", 0, n_head=3), mk("9x16x17-96-head16-nobias", (9, 16, 17), 1, 96, "none", 0, n_head=16, head_bias=False)]


@lru_cache(maxsize=None)
def all_cases() -> tuple:
    cs = _stream_cases() + _dma_cases() + _lds_chunk_cases() + _gemm_cases() + _conv_cases() + _dwmix_cases()
    assert len({c.id for c in cs}) == len(cs)
    return tuple(cs)


def cases(group: str) -> list:
    return [c for c in all_cases() if c.group == group]


# ------------------------------------------------------------------------------------------------------------- operands
def _rng(c: Case, salt: int) -> np.random.Generator:
    return np.random.default_rng([c.cin, c.chid, c.cout, c.N, c.rows, salt, int(c.family == "dense"), int(c.form == "folded")])


def _pick(rng, values, shape):
    return np.asarray(values, dtype=np.float64)[rng.integers(0, len(values), size=shape)]


def w3_pattern(chid: int, cout: int, rng) -> np.ndarray:
    """two non-zeros per hidden channel: outputs j mod C_out and (j mod C_out + 1 + j div C_out) mod C_out"""
    assert chid // cout + 1 < cout
    w3 = np.zeros((cout, chid))
    j = np.arange(chid)
    o1 = j % cout
    o2 = (o1 + 1 + j // cout) % cout
    w3[o1, j] = _pick(rng, (0.5, -0.5, 1.0, -1.0, 2.0, -2.0), chid)
    w3[o2, j] = _pick(rng, (0.5, -0.5, 1.0, -1.0, 2.0, -2.0), chid)
    return w3


@lru_cache(maxsize=64)
def _operands(key: tuple) -> dict:
    c = Case("", "", *key[:5], *key[5:])
    N, R, cin, chid, cout = c.N, c.rows, c.cin, c.chid, c.cout
    rng = _rng(c, 1)
    d = {}
    n_i, r_i = np.meshgrid(np.arange(N), np.arange(R), indexing="ij")
    if c.dims:
        # isolated +-1 voxels on a lattice of pitch 3 per channel (offset per channel, a quarter of the sites empty): at most ONE tap
        # reaches an output; taps +-1, bias +-1/2: the depthwise result is {0, +-1} + a half -- exact in fp32 and in bf16
        D, H, W = c.dims
        z, y, xx, ch = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), np.arange(cin), indexing="ij")
        site = ((z + ch) % 3 == 0) & ((y + ch // 3) % 3 == 0) & ((xx + ch // 9) % 3 == 0)
        x5 = np.where(site[None], _pick(rng, (1.0, -1.0, 1.0, 0.0), (N, D, H, W, cin)), 0.0)
        taps = _pick(rng, (1.0, -1.0), (27, cin))
        dwb = _pick(rng, (0.5, -0.5), cin)
        xt = torch.from_numpy(x5).permute(0, 4, 1, 2, 3)
        wt = torch.from_numpy(taps.T.reshape(cin, 1, 3, 3, 3).copy())
        reach = torch.nn.functional.conv3d(xt.abs(), torch.ones_like(wt), padding=1, groups=cin)
        assert float(reach.max()) == 1.0, "more than one tap reaches an output"
        conv = torch.nn.functional.conv3d(xt, wt, torch.from_numpy(dwb), padding=1, groups=cin).permute(0, 2, 3, 4, 1)
        x = conv.reshape(N, R, cin).numpy().copy()
        assert set(np.unique(np.abs(x)).tolist()) == {0.5, 1.5}
        d.update(x5=x5, taps=taps, dw_bias=dwb)
        w2 = np.zeros((chid, cin))
        j = np.arange(chid)
        w2[j, j % cin] = _pick(rng, (0.5, -0.5), chid)
        w2[j, (j + 1 + j // cin) % cin] = _pick(rng, (0.5, -0.5), chid)
    elif c.family == "sparse":
        x = np.zeros((N, R, cin))
        p1 = (r_i * 7 + n_i * 5) % cin
        p2 = (p1 + 1 + (r_i // cin + n_i) % (cin - 1)) % cin
        x[n_i, r_i, p1] = _pick(rng, (1.0, -1.0), (N, R))
        x[n_i, r_i, p2] = _pick(rng, (1.0, -1.0), (N, R))
        w2 = _pick(rng, (0.5, -0.5, 1.0, -1.0), (chid, cin))
    else:
        x = _pick(rng, (1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 0.0), (N, R, cin))
        w2 = np.zeros((chid, cin))
        j = np.arange(chid)
        k1 = j % cin
        k2 = (j + chid + 1 + j // cin) % cin if 2 * chid >= cin else (j + chid) % cin
        k2 = np.where(k2 == k1, (k1 + 1) % cin, k2)
        w2[j, k1] = _pick(rng, (0.5, -0.5, 1.0, -1.0), chid)
        w2[j, k2] = _pick(rng, (0.5, -0.5, 1.0, -1.0), chid)
    if c.conv:
        k = 2 * rng.integers(1024, 2048, size=chid) + 1              # 1 + k 2^-14 in (1.125, 1.25): |h| >= 1/8, where f16 ends at 2^-13
        b2 = 1.0 + k * 2.0 ** -14
    else:
        b2 = _pick(rng, (0.25, -0.25, 0.75, -0.75), chid)
    if c.form == "affine":
        a = _pick(rng, (0.5, 1.0, 2.0), (N, cin))
        b = _pick(rng, (0.0, 0.5, -0.5, 1.0, -1.0), (N, cin))
        if N > 1:                                    # no two samples share an affine
            for n in range(1, N):
                a[n, n % cin] = 2.0 if a[0, n % cin] != 2.0 else 0.5
        d["t"] = (x - b[:, None, :]) / a[:, None, :]
        d["ab"] = np.stack([a, b], 1)                # (N, 2, C_in)
        d["w2"], d["b2"] = w2, b2
    else:
        s = _pick(rng, (1.0, -1.0), (N, chid))
        s[:, 0] = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
        if N > 2:
            s[2, 1] = -s[0, 1]
        d["t"] = x
        d["ab"] = None
        d["w2"] = s[:, :, None] * w2[None]           # (N, C_hid, C_in)
        b2n = np.stack([np.roll(b2, n) for n in range(N)]) if c.conv else _pick(rng, (0.25, -0.25, 0.75, -0.75), (N, chid))
        d["b2"] = b2n
    d["x"] = x
    d["w3"] = w3_pattern(chid, cout, rng)
    q = np.arange(-8, 9) / 4.0
    d["b3"] = _pick(rng, q, cout)
    if c.dims and c.res == "add":
        d["res"] = d["x5"].reshape(N, R, cin)
    elif c.res in ("add", "up", "up_low"):
        d["res"] = _pick(rng, q, (N, R, cout))
    if c.res in ("up", "up_low"):
        d["res_bias"] = _pick(rng, q[q != 0], cout)
    if c.res == "up_low":
        d["res_low"] = _pick(rng, q[q != 0], (N, R // 8, cout))
    if c.res == "stem":
        d["x0"] = _pick(rng, np.arange(-3, 4), (N, R))
        d["stem_w"] = _pick(rng, (0.25, -0.25, 0.5, -0.5, 0.75, 1.25), cout)
        d["stem_b"] = _pick(rng, q, cout)
    if c.n_head:
        hw = _pick(rng, (0.0, 0.0, 1.0, -1.0, 2.0, -2.0), (c.n_head, 32))
        hw[np.arange(c.n_head), np.arange(c.n_head) * 2 % 32] = 1.0
        d["head_w"] = hw
        d["head_b"] = _pick(rng, q[q != 0], c.n_head) if c.head_bias else None
    if c.proj:
        d["proj_w"] = _pick(rng, (0.0, 0.0, 0.0, 1.0, -1.0, 2.0, -2.0), (32, 32))
        d["proj_b"] = _pick(rng, q[q != 0], 32)
    return d


def operands(c: Case) -> dict:
    """float64 numpy operands of a case (shared by the cases that differ in knobs only; treat as read-only)"""
    return _operands(c.data_key)


def _bf16_bits(v: np.ndarray) -> np.ndarray:
    """float64 -> bf16 bit patterns, round to nearest even; the value must be an fp32 number (so this is ONE rounding)"""
    v = np.asarray(v, dtype=np.float64)
    f = np.ascontiguousarray(v.astype(np.float32))
    assert (f.astype(np.float64) == v).all(), "not an fp32 number: float64 -> bf16 would round twice"
    b = f.view(np.uint32)
    return ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def to_bf16(v: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(_bf16_bits(v).view(np.int16)).view(BF16)


def bf16_np(v: np.ndarray) -> np.ndarray:
    return (_bf16_bits(v).astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def exact_sum(terms: np.ndarray, what: str) -> None:
    """terms (..., K): every sum over the last axis is exact in fp32 IN ANY ORDER -- per sum, all terms are multiples of 2^-k and
    sum |terms| < 2^24 * 2^-k"""
    terms = np.asarray(terms, dtype=np.float64).reshape(-1, terms.shape[-1])
    m, e = np.frexp(terms)
    M = np.abs(m * 2.0 ** 53).astype(np.int64)                       # the 53-bit significand as an integer
    low = (M & -M).astype(np.float64)                                # its lowest set bit
    lowexp = np.where(terms != 0, e - 53 + np.frexp(np.where(low > 0, low, 1.0))[1] - 1, 10000)
    unit = lowexp.min(1)                                             # per sum: every term is a multiple of 2^unit
    unit = np.where(unit == 10000, 0, unit)
    mag = np.abs(terms).sum(1) * 2.0 ** (-unit.astype(np.float64))
    worst = int(np.argmax(mag))
    assert mag[worst] < 2.0 ** EXACT_BITS, f"{what}: sum |terms| = {mag[worst]:.0f} units of 2^{unit[worst]} in sum {worst}: not below 2^24"


def upsample_parts(c: Case):
    """RES_UPSAMPLE: (face mask, res_low-position mask, index into res_low rows) per output row"""
    D, H, W = c.grid
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    face = (z == 0) | (y == 0) | (x == 0)
    oz, oy, ox = z - 1, y - 1, x - 1
    even = ~face & (((oz | oy | ox) & 1) == 0)
    low = ((oz >> 1) * (H // 2) + (oy >> 1)) * (W // 2) + (ox >> 1)
    return face.reshape(-1), even.reshape(-1), np.where(even, low, 0).reshape(-1)


@lru_cache(maxsize=64)
def _reference(key: tuple, train: bool) -> dict:
    c = Case("", "", *key[:5], *key[5:])
    d = _operands(key)
    N, R = c.N, c.rows
    out = {}
    w2 = d["w2"] if d["w2"].ndim == 3 else np.broadcast_to(d["w2"], (N,) + d["w2"].shape)
    b2 = d["b2"] if d["b2"].ndim == 2 else np.broadcast_to(d["b2"], (N,) + d["b2"].shape)
    if d["ab"] is not None:
        xe = d["t"] * d["ab"][:, 0][:, None, :] + d["ab"][:, 1][:, None, :]
        assert (xe == d["x"]).all() and (bf16_np(xe) == xe).all() and (bf16_np(d["t"]) == d["t"]).all()
    else:
        xe = d["t"]
    assert (bf16_np(w2) == w2).all()
    h = np.einsum("nrk,njk->nrj", xe, w2) + b2[:, None, :]
    out["h"] = h
    hin = h
    if train:
        out["hidden_pre"] = to_bf16(h)
        hin = out["hidden_pre"].double().numpy()
    g = gelu_h8_model(hin.astype(np.float32))
    assert (hin.astype(np.float32).astype(np.float64) == hin).all()
    out["g"] = g
    g64 = g.astype(np.float64)
    core = g64 @ d["w3"].T + d["b3"]
    res = np.zeros_like(core)
    if c.res == "add":
        res = d["res"]
    elif c.res == "stem":
        r = d["stem_w"][None, None, :] * d["x0"][:, :, None] + d["stem_b"][None, None, :]
        res = bf16_np(r)
        out["stem_unrounded"] = r
    y = core + res
    if c.res in ("up", "up_low"):
        face, even, low = upsample_parts(c)
        rl = np.broadcast_to(d["res_bias"], core.shape).copy()
        if c.res == "up_low":
            rl[:, even] = d["res_low"][:, low[even]]
        y = np.where(face[None, :, None], d["res"], core + rl + d["res"])
        out["rl"] = rl
    out["y64"] = y
    out["y"] = to_bf16(y)
    yb = out["y"].double().numpy()
    if c.n_head:
        lg = yb @ d["head_w"].T + (d["head_b"] if d["head_b"] is not None else 0.0)
        out["logits"] = torch.from_numpy(lg).float()
        assert torch.equal(out["logits"].double(), torch.from_numpy(lg))
    if c.proj:
        z = yb @ d["proj_w"].T + d["proj_b"]
        out["z64"] = z
        out["z"] = to_bf16(z)
    return out


def reference(c: Case, train: bool = False) -> dict:
    """h (fp64 pre-activation), g (the model's f16 hidden), y64 / y (bf16), and logits / z / hidden_pre where the case has them.
    train: the training forward -- GELU at the stored bf16(h)"""
    return _reference(c.data_key, train)


def min_trunc_diff(c: Case) -> int:
    """the least number of outputs on which truncation and round-to-nearest must differ: a sixteenth of the outputs that can hold a hidden
    term (min(C_out, 2 C_hid) per row); an eighth of that where the front faces of RES_UPSAMPLE take the skip value alone"""
    n = c.N * c.rows * min(c.cout, 2 * c.chid)
    return max(1, n // 128 if c.res in ("up", "up_low") else n // 16)


def assert_premises(c: Case, train: bool = False) -> dict:
    """The exactness premises of a case and its power to discriminate; -> the reference.  Host and GPU tests both call this."""
    return _assert_premises(c.data_key, train)


@lru_cache(maxsize=64)
def _assert_premises(key: tuple, train: bool) -> dict:
    c = Case("data", "-".join(str(k) for k in key), *key[:5], *key[5:])
    d, ref = operands(c), reference(c, train)
    N, R = c.N, c.rows
    h, g = ref["h"], ref["g"].astype(np.float64)
    w2 = d["w2"] if d["w2"].ndim == 3 else np.broadcast_to(d["w2"], (N,) + d["w2"].shape)
    b2 = d["b2"] if d["b2"].ndim == 2 else np.broadcast_to(d["b2"], (N,) + d["b2"].shape)
    # GEMM1: x holds integers (the fused block: halves), W2 halves, b2 multiples of 2^-14 (quarters outside the conversion cases): every term is a multiple of
    # 2^-14 and sum |terms| <= 4.75 < 2^24 * 2^-14
    assert (d["x"] * 2 == np.rint(d["x"] * 2)).all() and (w2 * 2 == np.rint(w2 * 2)).all() and (b2 * 2.0 ** 14 == np.rint(b2 * 2.0 ** 14)).all(), c.id
    nz = (np.einsum("nrk,njk->nrj", np.abs(d["x"]), np.abs(w2)) + np.abs(b2[:, None, :])).max()
    assert nz <= 4.75, (c.id, nz)                                                # sum |terms| of every pre-activation, all rows
    if c.conv:
        assert (np.abs(h) <= 4.0).all()
        h32 = h.astype(np.float32)
        assert (f32_to_f16_rtz(h32).astype(np.float64) != h).all() and (bf16_np(h) != h).all(), c.id
    else:
        assert (np.abs(h) <= 2.75).all() and ((h * 4) % 2 == 1).all(), f"{c.id}: pre-activations must be odd quarters within 2.75"
    # GEMM2 + epilogue: every output element
    nzc = np.abs(d["w3"]).sum(0) > 0
    assert nzc.all(), f"{c.id}: hidden channels {np.nonzero(~nzc)[0][:8]} feed no output"
    K = int((d["w3"] != 0).sum(1).max())
    idx = np.argsort(d["w3"] == 0, axis=1, kind="stable")[:, :K]                 # per output row: its non-zero columns first
    w3k = np.take_along_axis(d["w3"], idx, 1)                                    # (C_out, K), zero padded
    for n in range(N):
        terms = g[n][:, idx] * w3k[None]                                         # (R, C_out, K): the non-zero products of every output
        extra = [np.broadcast_to(d["b3"][None, :, None], terms.shape[:2] + (1,))]
        if c.res == "add":
            extra.append(d["res"][n][:, :, None])
        elif c.res == "stem":
            r = ref["stem_unrounded"][n]
            assert (r.astype(np.float32).astype(np.float64) == r).all()
            extra.append(bf16_np(r)[:, :, None])
        elif c.res in ("up", "up_low"):
            extra += [d["res"][n][:, :, None], ref["rl"][n][:, :, None]]
        exact_sum(np.concatenate([terms] + extra, -1), f"{c.id}: GEMM2 + epilogue, sample {n}")
    pat = {tuple(np.round(d["w3"][:, j] * 2).astype(int).tolist()) for j in range(c.chid)}
    assert len(pat) == c.chid, f"{c.id}: two hidden channels share a projection pattern"
    yb = ref["y"].double().numpy()
    if c.n_head:
        hb = d["head_b"] if d["head_b"] is not None else np.zeros(c.n_head)
        terms = yb[:, :, None, :] * d["head_w"][None, None]
        exact_sum(np.concatenate([terms, np.broadcast_to(hb[None, None, :, None], terms.shape[:3] + (1,))], -1), f"{c.id}: head")
    if c.proj:
        terms = yb[:, :, None, :] * d["proj_w"][None, None]
        exact_sum(np.concatenate([terms, np.broadcast_to(d["proj_b"][None, None, :, None], terms.shape[:3] + (1,))], -1), f"{c.id}: projection")
    # the tensor discriminates: truncation against round-to-nearest, and every hidden chunk matters
    live = np.ones((R,), bool)
    if c.res in ("up", "up_low"):
        live = ~upsample_parts(c)[0]
    ybits = _bf16_bits(ref["y64"][:, live])
    f32bits = np.ascontiguousarray(ref["y64"][:, live].astype(np.float32)).view(np.uint32)
    ntr = int(((f32bits >> np.uint32(16)).astype(np.uint16) != ybits).sum())
    assert ntr >= min_trunc_diff(c), f"{c.id}: truncation differs from round-to-nearest on {ntr} outputs only (need {min_trunc_diff(c)})"
    gl, yl = g[:, live], ref["y64"][:, live]
    for hc in range(c.chid // 32):
        sl = slice(hc * 32, hc * 32 + 32)
        touched = np.abs(d["w3"][:, sl]).sum(1) > 0                              # the outputs this chunk feeds
        without = yl[:, :, touched] - gl[:, :, sl] @ d["w3"][touched][:, sl].T
        assert (_bf16_bits(without) != ybits[:, :, touched]).any(), f"{c.id}: dropping hidden chunk {hc} changes no output"
    return ref


def check_bits(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    """bit equality over the whole tensor (the one assertion of the GPU suite; the host proof makes it of its restatements); on failure
    the count and the first differing elements"""
    got = got.detach().cpu()
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), f"{what}: {got.dtype} {tuple(got.shape)} / {want.dtype} {tuple(want.shape)}"
    it = torch.int16 if got.element_size() == 2 else torch.int32
    gb, wb = got.contiguous().view(it), want.contiguous().view(it)
    if torch.equal(gb, wb):
        return
    idx = (gb != wb).nonzero()
    first = [f"{tuple(i.tolist())} got {float(got[tuple(i)])!r} want {float(want[tuple(i)])!r}" for i in idx[:6]]
    raise AssertionError(f"{what}: {len(idx)} of {got.numel()} elements differ (exact operands: none may); last-axis indices "
                         f"{sorted(set(idx[:, -1].tolist()))[:16]}; first: " + "; ".join(first))


def paired_row(T: int, m: int) -> int:
    return (T >> 1) * 32 + (m >> 2) * 8 + (T & 1) * 4 + (m & 3)

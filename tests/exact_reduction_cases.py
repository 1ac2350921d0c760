"""Exact-arithmetic cases for the split-slot reductions of the training kernels (weight / bias gradients, channel statistics,
LayerNorm parameter gradients).

The operands are bf16 / fp32 values in {-s, 0, s} for a power of two s, with a seeded sparsity.  Every product is then exact in fp32,
and as long as the sum of the magnitudes of the terms of one output stays below 2^24 quanta, so is every partial sum in whatever order
and grouping a kernel adds them.  The correct fp32 result is the fp64 sum bit for bit: a dropped, doubled or misrouted row or slot shows
up as a nonzero difference with zero tolerance.  Where a quantity cannot be made exact (LayerNorm x-hat) the check is against fp64 with
the derived bound (L + S + 2) 2^-24 sum|t| (L rows per slot, S slots), and the case shows that losing the last slot exceeds twice it.

Plain module (no tests): the GPU cases (test_gpu_exact_reductions.py) and the CPU checks (test_host_exact_reduction_cases.py) import it.
The slot-count mirrors restate the dispatchers' host arithmetic (csrc/train_kernels.hip, colstats.h, dwconv_kernels.hip,
upcat_kernels.hip, transformer_kernels.hip, swin_kernels.hip); the GPU cases assert that the library reports the same counts."""
from __future__ import annotations

from dataclasses import dataclass, field

import torch

EXACT_F32 = 2 ** 24          # integers up to here (in units of the quantum) are exact in fp32
EXACT_F16 = 2 ** 11          # ... and in fp16 (the nine-tap dwconv statistics keep fp16 partials)
U32 = 2.0 ** -24             # unit roundoff of fp32 (round to nearest)


# ---------------------------------------------------------------------------------------------------------------- operands
def ternary(shape, density: float, seed: int, *, scale: float = 1.0, dtype=torch.bfloat16, device="cpu",
            row_density=None) -> torch.Tensor:
    """Values in {-scale, 0, +scale}, nonzero with probability `density` (half of them negative), seeded.  row_density: optional
    (rows,) fp32 tensor of per-row densities over the leading len(shape)-1 axes flattened (overrides `density`)."""
    g = torch.Generator(device=device).manual_seed(int(seed))
    u = torch.rand(shape, generator=g, device=device, dtype=torch.float32)
    d = density
    if row_density is not None:
        d = row_density.to(device=device, dtype=torch.float32).view(*shape[:-1], 1)
    v = (u < d).to(torch.float32) - 2.0 * (u < 0.5 * d).to(torch.float32)
    if scale != 1.0:
        v.mul_(scale)
    return v.to(dtype)


def binary(shape, density: float, seed: int, *, value: float, dtype=torch.bfloat16, device="cpu") -> torch.Tensor:
    """Values in {0, value}, `value` with probability `density`, seeded (GELU pre-activations in {0, 16})."""
    g = torch.Generator(device=device).manual_seed(int(seed))
    u = torch.rand(shape, generator=g, device=device, dtype=torch.float32)
    return ((u < density).to(torch.float32) * value).to(dtype)


def tail_dense_rows(rows: int, tail: int, sparse: float, dense: float = 1.0) -> torch.Tensor:
    """Per-row densities: `sparse` everywhere except the last `tail` rows (`dense`): the last slot then carries a signal that a
    derived rounding bound over all rows cannot hide."""
    d = torch.full((rows,), float(sparse), dtype=torch.float32)
    d[rows - tail:] = dense
    return d


def exact_affine(N: int, C: int, seed: int) -> torch.Tensor:
    """Per-sample norm affine (N, 2, C) fp32 with a in {+-1, +-2, +-1/2} and b in {-2 .. 2}: a*x + b of a ternary x is exact in fp32
    and in bf16, in any evaluation order (fma or not)."""
    g = torch.Generator().manual_seed(int(seed))
    avals = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5, -0.5])
    a = avals[torch.randint(0, 6, (N, C), generator=g)]
    b = torch.randint(-2, 3, (N, C), generator=g).to(torch.float32)
    return torch.stack([a, b], 1).contiguous()


def is_bf16_exact(t: torch.Tensor) -> bool:
    return bool(torch.equal(t.float().bfloat16().float(), t.float()))


# ---------------------------------------------------------------------------------------------------------------- caps and bounds
def assert_exact_cap(abs_sum: float, quantum: float, cap: int = EXACT_F32, what: str = "") -> None:
    """Every partial of a sum whose terms are multiples of `quantum` with sum|t| = abs_sum is exact below cap quanta."""
    q = float(abs_sum) / float(quantum)
    assert q < cap, f"{what}: sum|t| = {abs_sum} is {q:.3g} quanta of {quantum}, over the exactness cap {cap}: reshape the case"


def gemm_abs_bound(a_absmax: float, colsum_abs: torch.Tensor) -> float:
    """sum_r |a_rk| |b_ro| <= max|a| * max_o sum_r |b_ro|: a cheap, sound bound of every output's sum|t| of a^T b."""
    return float(a_absmax) * float(colsum_abs.max())


def slot_rounding_bound(rows_per_slot: int, slots: int, abs_sum) -> torch.Tensor | float:
    """|fp32 slot-split sum - exact| <= (L + S + 2) u sum|t| (L terms per slot in sequence, S slot partials, +2 for the rounding of
    each term's factors): the standard recursive-summation bound, to first order."""
    return (rows_per_slot + slots + 2) * U32 * abs_sum


def slot_rows(rows_total: int, slots: int):
    """[(start, stop)) of each slot of a ceil-divided row split (every dispatcher here splits rows that way)."""
    rps = -(-rows_total // slots)
    return [(s * rps, min(rows_total, (s + 1) * rps)) for s in range(slots) if s * rps < rows_total]


def split_facts(rows_per_sample: int, N: int, slots: int) -> dict:
    """Slot layout facts of a flat row split over N samples: ragged last slot, a slot that straddles a sample boundary."""
    total = rows_per_sample * N
    sl = slot_rows(total, slots)
    rps = sl[0][1] - sl[0][0]
    straddle = any((a // rows_per_sample) != ((b - 1) // rows_per_sample) for a, b in sl)
    return dict(slots=len(sl), rows_per_slot=rps, ragged=(sl[-1][1] - sl[-1][0]) != rps, straddle=straddle, last=sl[-1])


# ---------------------------------------------------------------------------------------------------------------- slot emulation
def slot_split_sum_f32(terms: torch.Tensor, slots: int, *, drop=None, double=None) -> torch.Tensor:
    """CPU emulation of a slot-split fp32 reduction over axis 0 of `terms` (rows, n): each slot summed in row order in fp32, then
    the slot partials in slot order in fp32.  drop / double: a slot index to lose / to count twice (fault models)."""
    parts = []
    for s, (a, b) in enumerate(slot_rows(terms.shape[0], slots)):
        acc = torch.zeros(terms.shape[1:], dtype=torch.float32)
        for r in range(a, b):
            acc = acc + terms[r].float()
        if s == drop:
            continue
        parts.append(acc)
        if s == double:
            parts.append(acc)
    out = torch.zeros(terms.shape[1:], dtype=torch.float32)
    for p in parts:
        out = out + p
    return out


# ---------------------------------------------------------------------------------------------------------------- GELU forms
def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


def gelu_erf_f32(x: torch.Tensor) -> torch.Tensor:
    """fp32 restatement of gelu_erf (csrc/pytc_common.h: Abramowitz-Stegun 7.1.26, exp2 / rcp as correctly rounded fp32 ops)."""
    x = x.float()
    az = x.abs() * _f32(0.70710678118654752440)
    t = 1.0 / (_f32(0.3275911) * az + 1.0)
    p = t * _f32(1.061405429) + _f32(-1.453152027)
    p = t * p + _f32(1.421413741)
    p = t * p + _f32(-0.284496736)
    p = t * p + _f32(0.254829592)
    p = p * t
    pe = p * torch.exp2(-az * az * _f32(1.44269504088896340736))
    one_plus_erf = torch.where(x < 0, pe, 2.0 - pe)
    return 0.5 * x * one_plus_erf


def gelu_fast_f32(x: torch.Tensor) -> torch.Tensor:
    """fp32 restatement of gelu_fast (the sigmoid form of the bf16 fast paths and of gelu_fast_with_grad)."""
    x = x.float()
    x2 = torch.clamp(x * x, max=64.0)
    p = x2 * _f32(1.0142630e-3) + _f32(-1.0677572e-1)
    p = p * x2 + _f32(-2.3011213)
    e = torch.exp2(x * p)
    return x * (1.0 / (1.0 + e))


def gelu_fast_with_grad_f32(x: torch.Tensor):
    """fp32 restatement of gelu_fast_with_grad: (gelu_fast(x), its derivative)"""
    x = x.float()
    x2 = torch.clamp(x * x, max=64.0)
    p = x2 * _f32(1.0142630e-3) + _f32(-1.0677572e-1)
    p = p * x2 + _f32(-2.3011213)
    e = torch.exp2(x * p)
    s = 1.0 / (1.0 + e)
    g = x * s
    q = x2 * _f32(2.0 * 1.0142630e-3) + _f32(-1.0677572e-1)
    du = (x2 + x2) * q + p
    return g, (g * (1.0 - s)) * (du * _f32(-0.69314718055994530942)) + s


GELU_FORMS = {"erf": gelu_erf_f32, "fast": gelu_fast_f32}
GELU_EXACT_VALUES = (0.0, 16.0)      # pre-activations whose GELU is the value itself (16) or 0 under every form, after bf16 rounding


# ---------------------------------------------------------------------------------------------------------------- slot-count mirrors
def pw_wgrad_slots(rows_total: int) -> int:
    return max(1, min(1024, rows_total // 256))


def _wg_tile16(c: int) -> int:
    return 4 if c % 64 == 0 else (2 if c % 32 == 0 else (1 if c % 16 == 0 else 0))


def wgrad_mfma_slots(rows_total: int, c_in: int, c_out: int, *, whole_rounds: bool = True, small_split: bool = True) -> int:
    """Row slots of the bf16 MFMA weight-gradient launch (train_kernels.hip wgrad_mfma_slots)."""
    slots = pw_wgrad_slots(rows_total)
    mt, nt = _wg_tile16(c_out), _wg_tile16(c_in)
    tiles = (c_out // (16 * mt)) * (c_in // (16 * nt))
    want = rows_total // 2048
    cap = 1024 // tiles if 1024 // tiles > 1 else 1
    want = 1 if want < 1 else min(want, cap)
    per_cu = 2 if mt * nt >= 8 else (3 if mt * nt >= 4 else 4)
    resident = 256 * per_cu // tiles
    if whole_rounds and resident >= 8 and want > resident:
        want = (want // resident) * resident
    if small_split and want * tiles < 512:
        more = min(512 // tiles, rows_total // 256)
        want = max(want, more)
    return min(want, slots)


def pw_launch_slots(rows_total: int, c_in: int, c_out: int, bf16: bool = True, **knobs) -> int:
    """Slots a pw_wgrad launch writes (bf16 with channel counts in multiples of 16: the MFMA count, else the workspace bound)."""
    if bf16 and _wg_tile16(c_in) and _wg_tile16(c_out):
        return wgrad_mfma_slots(rows_total, c_in, c_out, **knobs)
    return pw_wgrad_slots(rows_total)


def mixer_bwd_rc_sps(N: int, rows_per_sample: int, c_hid: int, *, slot_div: int = 1) -> int:
    """row slots per sample of pytc_mixer_bwd_rc (C = C_out = 32; knob mixer_bwd_rc_slot_div)"""
    slots = wgrad_mfma_slots(N * rows_per_sample, c_hid, 32)
    if slot_div > 1 and slots // slot_div >= 512:
        slots //= slot_div
    return max(1, slots // N)


def pw_wgrad_groupnorm_sps(N: int, rows_per_sample: int, C: int, c_hid: int) -> int:
    """row slots per sample of pytc_pw_wgrad_groupnorm"""
    return max(1, wgrad_mfma_slots(N * rows_per_sample, C, c_hid) // N)


def colstats_slots(rows: int) -> int:
    return max(1, min(1024, rows // 64))


def dw_wgrad_form(gdims, xdims, C: int, K: int, stride: int, *, march: bool = True, vec: bool = True) -> str:
    """Which form pytc_dw_wgrad dispatches to (bf16): 'march', 'vec' or 'generic'."""
    D, H, W = gdims
    if march and tuple(gdims) == tuple(xdims) and K == 3 and stride == 1 and C % 32 == 0 and D >= 8 and H >= 16 and W >= 16 \
            and H * W * C < (1 << 30):
        return "march"
    if vec and K == 3 and C % 8 == 0 and C // 8 <= 256:
        return "vec"
    return "generic"


def dw_wgrad_slots(N: int, gdims, xdims, C: int, K: int, stride: int, *, march: bool = True, vec: bool = True, ppl: int = 0) -> int:
    """Total slots (all samples) of pytc_dw_wgrad in bf16 (train_kernels.hip make_wg_vec / make_wg, dwconv_kernels.hip march)."""
    form = dw_wgrad_form(gdims, xdims, C, K, stride, march=march, vec=vec)
    D, H, W = gdims
    vg = D * H * W
    if form == "march":
        ty, tx = -(-H // 8), -(-W // 8)
        fp = ty * tx * (C // 32) * N
        nzc = max(1, -(-2048 // fp))
        nzc = min(nzc, max(1, D // 14))
        zc = -(-D // nzc)
        return ty * tx * (-(-D // zc)) * N
    if form == "vec":
        PL = 256 // (C // 8)
        if ppl <= 0:
            ppl = min(16, max(4, vg * N * 3 // (PL * 1024)))
        sl = -(-vg // (PL * ppl))
        return max(1, min(1024, sl)) * N
    for v in (4, 2, 1):
        if C % v == 0 and C // v <= 256:
            break
    vs = 256 // (C // v)
    it = max(1, min(256, vg // (vs * 64)))
    return -(-vg // (vs * it)) * N


def upcat_wgrad_splits(rows: int, C_in: int, C_u: int, bf16: bool = True) -> int:
    ks = 32 if bf16 else 16
    tiles = -(-(C_in + 1) // 64) * -(-(8 * C_u) // 64)
    s = -(-512 // tiles)
    s = min(s, min(64, -(-rows // ks)))
    return max(s, 1)


def layernorm_wide_slots(rows: int) -> int:
    return -(-rows // 32)


def layernorm_any_slots(rows: int) -> int:
    return -(-rows // 256)


def layernorm_rows_rpb(C: int) -> int:
    """rows per block of layernorm_rows_bwd (norm_variant_kernels.hip ln_vec: C = VEC * 2^k, VEC <= 8, 2^k <= 64); 0 = unsupported"""
    for v in (8, 4, 2, 1):
        k = C // v
        if C % v == 0 and k >= 1 and (k & (k - 1)) == 0 and k <= 64:
            return 256 // k
    return 0


def layernorm_rows_slots(rows: int, C: int) -> int:
    """blocks (= partial slots) of layernorm_rows_bwd, at most 1024: beyond that each block strides over the row blocks"""
    rpb = layernorm_rows_rpb(C)
    return min(1024, -(-rows // rpb)) if rpb and rows >= 1 else 0


def slot_order_sum(part: torch.Tensor) -> torch.Tensor:
    """fp32 sum of part[0] + part[1] + ... in slot order"""
    out = torch.zeros_like(part[0])
    for s in range(part.shape[0]):
        out = out + part[s]
    return out


# ---------------------------------------------------------------------------------------------------------------- the shapes
MEDNEXT_N = 4
MEDNEXT_SIDE = 112
MEDNEXT_C = 32


def mednext_levels():
    """(level, side, C) of MedNeXt-S at its 4 x 112^3 training window: C 32 -> 512, hidden 2 C."""
    return [(lv, MEDNEXT_SIDE >> lv, MEDNEXT_C << lv) for lv in range(5)]


@dataclass
class PwCase:
    name: str
    N: int
    rows: int                 # rows per sample
    c_in: int
    c_out: int
    ab: bool = False          # per-sample norm affine on x
    gelu: bool = False        # x_act = GELU (x in {0, 16})
    density_x: float = 0.5
    density_dy: float = 0.25
    knobs: dict = field(default_factory=dict)

    @property
    def slots(self) -> int:
        kn = {k: bool(v) for k, v in self.knobs.items() if k in ("whole_rounds", "small_split")}
        return pw_launch_slots(self.N * self.rows, self.c_in, self.c_out, **kn)


def pw_cases():
    """MedNeXt-S expand (C -> 2C, norm affine on x) and project (2C -> C, GELU operand) weight gradients at levels 0-4 of the
    4 x 112^3 step, the odd batches of the odd-shape tests (3 x 32x48x64 and 5 x 16x80x48 at level 0) and a ragged odd shape.
    At the production sizes the row split is even and aligned to the samples (4 x 112^3 = 1024 slots x 5488 rows, 112^3 = 256 x 5488):
    ragged last slots and slots across a sample boundary come from the odd shapes, and each case ID says which it has."""
    out = []
    for lv, side, C in mednext_levels():
        r = side ** 3
        out.append(PwCase(f"L{lv}_expand_{C}x{2 * C}_ab", MEDNEXT_N, r, C, 2 * C, ab=True))
        out.append(PwCase(f"L{lv}_project_{2 * C}x{C}_gelu", MEDNEXT_N, r, 2 * C, C, gelu=True))
    out.append(PwCase("odd_N3_32x48x64_expand_ab", 3, 32 * 48 * 64, 32, 64, ab=True))
    out.append(PwCase("odd_N5_16x80x48_project_gelu", 5, 16 * 80 * 48, 64, 32, gelu=True))
    # a shape whose row split is ragged as well: 3 x 33x47x61
    out.append(PwCase("odd_N3_33x47x61_expand_ab", 3, 33 * 47 * 61, 32, 64, ab=True))
    out.append(PwCase("odd_N3_33x47x61_project_gelu", 3, 33 * 47 * 61, 64, 32, gelu=True))
    return out


def pw_case_abs_bound(c: PwCase) -> tuple[float, float]:
    """(expected sum|t| of the largest dW output with a 5 % margin, quantum): max|x| times the expected nonzero dy rows.  The GPU
    case asserts the cap on the drawn operands themselves; this is the shape-level check that the densities fit."""
    xmax = 16.0 if c.gelu else (4.0 if c.ab else 1.0)                       # |a x + b| <= 2 + 2
    quantum = 16.0 if c.gelu else (0.5 if c.ab else 1.0)                    # a = 1/2 halves the grid; GELU operands are 0 / 16
    return 1.05 * xmax * c.density_dy * c.N * c.rows, quantum


@dataclass
class DwCase:
    name: str
    N: int
    gdims: tuple
    xdims: tuple
    C: int
    stride: int
    kind: str                 # block | down | up (the call shapes of training/autograd.py _dw_backward)


def dw_cases():
    out = []
    for lv, side, C in mednext_levels():
        out.append(DwCase(f"L{lv}_block_C{C}", MEDNEXT_N, (side,) * 3, (side,) * 3, C, 1, "block"))
        if lv < 4:
            h = side // 2
            out.append(DwCase(f"L{lv}_down_C{C}", MEDNEXT_N, (h,) * 3, (side,) * 3, C, 2, "down"))
            # up block into level lv: the transposed depthwise conv on level lv+1's channels; g = the small input, x = the compact
            # (2 h - 1)^3 gradient grid
            C1 = C * 2
            out.append(DwCase(f"L{lv}_up_C{C1}", MEDNEXT_N, (h,) * 3, (2 * h - 1,) * 3, C1, 2, "up"))
    out.append(DwCase("odd_N3_32x48x64_block_C32", 3, (32, 48, 64), (32, 48, 64), 32, 1, "block"))
    out.append(DwCase("odd_N5_16x80x48_down_C32", 5, (8, 40, 24), (16, 80, 48), 32, 2, "down"))
    return out

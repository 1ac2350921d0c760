"""Exact-arithmetic cases for the train-step epilogue (csrc/loss_optim_kernels.hip, csrc/cldice_kernels.hip, training/fused.py): the
fused BCE + Dice loss and its gradient, the multi-tensor gradient norm / clip / AdamW / EMA update, the tile-partial sums of
SoftClDiceLoss.  Same method as exact_reduction_cases.py, whose helpers (EXACT_F32, U32, assert_exact_cap, slot_rows, tail_dense_rows,
slot_split_sum_f32, ternary) are imported, not restated.

Fused loss operands.  Family 1: logits in {-128, +128}: __expf gives exactly 0 or +inf, so p = sigmoid is exactly 0 or 1, log1pf(0) = 0
and the bce term is 0, 128 or 128 pos_weight.  Targets in {0, 1}, weights in {0, 1/2, 1, 2}, pos_weight in {None, 1/2, 2}: every term
of the five sums is a multiple of a power-of-two quantum, and below EXACT_F32 quanta of sum|t| every partial sum is exact in fp32 in
any order: `sums` must equal the fp64 sums bit for bit.  Family 2 adds logit 0 (p = 1/2 exactly, bce = ln 2 * lw NOT exact): used with
w_bce = 0 only, sums 1..4 asserted.  A voxel is "wrong" (bce != 0) with a small probability everywhere except in the rows of the last
slot, where every other voxel is wrong (tail_dense_rows with density 1/2, so that sum p t of the slot is not zero either): a lost or
doubled last slot is a large integer.

Derived bounds (u = U32 = 2^-24, gamma(k) = k u / (1 - k u); a correctly rounded operation costs 1 u, a division or square root is
counted as 4 u = 2 ulp, not assumed correctly rounded):

* LOSS_BCE_U = 5: bce = numerator / den: the numerator is exact (global cap), den is exact or rounded once (N C R > 2^24), one
  division.
* LOSS_DICE_U = 23: per (n, c) q = (2 s2 + e_nr) / (s3 + s4 + e_dr): e_nr, e_dr as fp32 (2), the two additions (2; all 0 for dyadic
  smoothing under the cap), the division (4); 1 - q (1): 9 u absolute as q <= 1 + 2u.  The block tree adds N C <= 256 such terms in 8
  levels: 8 u each term.  The mean's division: 4, two spare for the terms slightly over 1.  Absolute, the dice term being <= 1.
* LOSS_U = LOSS_DICE_U + LOSS_BCE_U + 4 = 32: the two products by w_bce, w_dice and their sum (3) and the rounding of the result:
  |loss - ref| <= gamma(32) (w_bce |bce| + w_dice).
* BWD_BCE_U = 6: dx = kb w (p lw - pw t) with kb = fl(fl(go w_bce) / den): den rounded once at most (1), the product (1), the division
  (4); w is a power of two and (p lw - pw t) is 0, 1 or -pw: those products are exact, and the Dice part is exactly 0 (p (1-p) = 0).
* BWD_DICE_U = 10: dx = kd (I2 - 2 t Dn) / 4 with kd = fl(fl(go w_dice) / fl(fl(NC Dn) Dn)): I2, Dn exact under the cap; three products
  (3), the division (4), I2 - 2 t Dn may pass 2^24 quanta (1), the product by kd (1), the sum with the (zero) bce part (1).
* NORM_U = 4: last_grad_norm = sqrtf(S) of the exact integer S: one square root.  CLIP_U = 7: max_norm / (norm + 1e-6f): the
  constant (1), max_norm as fp32 (1), the addition (1), the division (4).
* AdamW (adamw_ref64; M = |b1 m| + |(1-b1) g c|, V = b2 v + (1-b2) (g c)^2, both sums of the magnitudes; the reference takes the fp32
  scalar row the ABI receives, in which 1 - beta is exact by Sterbenz' lemma):
  m' : gamma(3) M        (g c: 1, its product: 1, the sum: 1; the b1 m term has 2)
  v' : gamma(5) V        (g c twice: 2, two products: 2, the sum: 1)
  p' : gamma(4) |p| + gamma(25) U, U = step M / den (the update with |m'| replaced by M, which covers cancellation in m'):
       decay p (1 - lr wd): 1 - lr wd (2), product (1), final subtraction (1): 4 on |p|.  Update: step = lr / bc1 (4), m' (3), its
       product (1); den = sqrtf(v') / bc2s + eps: v' (5/2 after the root), sqrtf (4), division (4), sum (1) = 12 with rounding up;
       the division by den (4); the final subtraction (1): 25.
  ema': gamma(3) (|d e| + |(1-d) p'|) + (1 - d) bound(p')
  plus one fp32 minimum normal (2^-126) everywhere, for flushed underflow.
* clDice: binary prob / target make the skeleton binary, weights in {0, 1/2, 1, 2} make each term a multiple of 1/4: exact, tolerance 0.

Plain module (no tests): test_gpu_exact_epilogue.py and test_host_epilogue_exact_cases.py import it."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn.functional as F

from exact_reduction_cases import EXACT_F32, U32, assert_exact_cap, slot_rows, tail_dense_rows  # noqa: F401

LOSS_BCE_U, LOSS_DICE_U, LOSS_U = 5, 23, 32
BWD_BCE_U, BWD_DICE_U = 6, 10
NORM_U, CLIP_U = 4, 7
F32_MIN_NORMAL = 2.0 ** -126
LOGIT = 128.0


def gamma(k: float) -> float:
    """k roundings to first and higher order: k u / (1 - k u)"""
    return k * U32 / (1.0 - k * U32)


# ---------------------------------------------------------------------------------------------------------------- fused loss: mirrors
def loss_slots(R: int) -> int:
    """csrc/loss_optim_kernels.hip loss_slots: row slots of one (sample, channel)"""
    return max(1, min(256, R // 16384))


def loss_ws_elems(N: int, C: int, R: int) -> int:
    return loss_slots(R) * N * C * 5


def loss_bwd_blocks(R: int) -> int:
    """blocks per (n, c) of the backward launch, 1024 rows each; past 2048 blocks every block strides further"""
    return min(-(-R // 1024), 2048)


def loss_bwd_passes(R: int) -> int:
    """grid-stride iterations of the busiest thread of bce_dice_bwd_kernel"""
    return -(-R // (loss_bwd_blocks(R) * 256))


OPT_CHUNK = 4096
OPT_MAX_ROWS = 8
CLD_TILE = 1024


def opt_chunks(numel: int) -> int:
    return -(-numel // OPT_CHUNK)


def cldice_tiles(voxels: int) -> int:
    return -(-voxels // CLD_TILE)


# ---------------------------------------------------------------------------------------------------------------- fused loss: cases
@dataclass(frozen=True)
class LossCase:
    name: str
    N: int
    C: int
    spatial: tuple
    pw: Optional[float] = None
    weight: str = "full"            # none | full (N, C, ...) | bcast (N, 1, ...): stride_c = 0
    wvals: tuple = (0.0, 0.5, 1.0, 2.0)
    layout: str = "contig"          # contig | cl (channels-last memory viewed as NC...) | cl_slice (channels of a wider channels-last
    #                                 holder) | crop (a spatial crop of a larger contiguous tensor: strides do not collapse, _prep copies)
    tdtype: str = "float"           # float | uint8 | bool
    family: int = 1                 # 2: logit 0 as well; w_bce must be 0
    w_bce: float = 1.0
    w_dice: float = 1.0
    snr: float = 1.0
    sdr: float = 1.0
    wrong: float = 1.0 / 64         # probability of a wrong (bce != 0) voxel outside the last slot
    go: float = 1.0                 # upstream gradient (a power of two)

    @property
    def R(self) -> int:
        return math.prod(self.spatial)

    @property
    def slots(self) -> int:
        return loss_slots(self.R)

    @property
    def den_rounded(self) -> bool:
        """no weight map and N C R > 2^24: the bce denominator float(N C) * float(R) is rounded once"""
        return self.weight == "none" and self.N * self.C * self.R > EXACT_F32

    @property
    def id(self) -> str:
        sl = slot_rows(self.R, self.slots)
        ragged = len(sl) > 1 and (sl[-1][1] - sl[-1][0]) != (sl[0][1] - sl[0][0])
        return (f"{self.name}-N{self.N}C{self.C}-R{self.R}-slots{self.slots}" + ("-ragged" if ragged else "")
                + f"-bwd{loss_bwd_passes(self.R)}pass" + ("-den_rounded" if self.den_rounded else ""))


def loss_cases():
    """R around the 1 -> 2 slot switch, the production windows (112^3 = 85 slots ragged, 18/24 x 256^2 = 72 / 96 slots, 160^3 = 250
    slots and > 4 backward passes, 170 x 168 x 168 = the 256-slot cap with a ragged last slot), R around the backward's 2048-block cap,
    a 2-D case, every layout and target dtype at 112^3, family 2 (Dice gradient) at 112^3 and 160^3, the default 1e-5 smoothing.
    N C R > 2^24 without a weight map in `unweighted_big` (see den_rounded: stated in the ID)."""
    c = []
    edge_shapes = {16383: (3, 43, 127), 16384: (16, 32, 32), 32767: (7, 31, 151), 32768: (32, 32, 32), 32769: (9, 11, 331)}
    for i, (R, sp) in enumerate(edge_shapes.items()):
        c.append(LossCase(f"edge{R}", 2, 2, sp, pw=(None, 0.5, 2.0)[i % 3], weight=("full", "bcast", "none")[i % 3]))
    c.append(LossCase("edge32769_dice", 2, 2, (9, 11, 331), family=2, w_bce=0.0))
    c.append(LossCase("w112", 4, 1, (112,) * 3))
    c.append(LossCase("w112_default_smooth", 4, 1, (112,) * 3, pw=2.0, snr=1e-5, sdr=1e-5))
    c.append(LossCase("w112_cl_bcast", 4, 3, (112,) * 3, pw=2.0, weight="bcast", layout="cl"))
    c.append(LossCase("w112_cl_slice_u8", 2, 3, (112,) * 3, pw=0.5, layout="cl_slice", tdtype="uint8"))
    c.append(LossCase("w112_crop_bool", 2, 1, (112,) * 3, pw=0.5, layout="crop", tdtype="bool", go=0.5))
    c.append(LossCase("w112_unweighted_big", 4, 3, (112,) * 3, weight="none", layout="cl"))
    c.append(LossCase("w112_dice", 2, 2, (112,) * 3, family=2, w_bce=0.0, layout="cl"))
    c.append(LossCase("w18x256", 2, 1, (18, 256, 256), pw=2.0))
    c.append(LossCase("w24x256", 2, 1, (24, 256, 256), weight="none"))
    c.append(LossCase("below_2pow21", 1, 2, (49, 127, 337)))
    c.append(LossCase("above_2pow21", 1, 2, (9, 43, 5419), pw=2.0))
    c.append(LossCase("w160", 1, 2, (160,) * 3, pw=0.5, wvals=(0.0, 0.5, 1.0)))
    c.append(LossCase("w160_dice", 1, 2, (160,) * 3, family=2, w_bce=0.0, go=2.0))
    c.append(LossCase("cap256", 1, 2, (170, 168, 168), pw=0.5, wvals=(0.0, 0.5, 1.0), weight="bcast"))
    c.append(LossCase("plane1024x768", 2, 3, (1024, 768), pw=2.0, layout="cl"))
    return c


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(int(seed))


def loss_operands(c: LossCase, seed: Optional[int] = None):
    """-> (logits, target, weight or None) as CPU tensors in logical (N, C, *spatial) order (weight (N, 1, ...) when broadcast); logits
    fp32 in {-128, 128} (family 2: and 0), target in {0, 1} as c.tdtype, weight fp32 from c.wvals.  Seeded by the case."""
    seed = (c.R * 31 + c.N * 7 + c.C) if seed is None else seed
    g = _gen(seed)
    shape = (c.N, c.C, c.R)
    t = torch.rand(shape, generator=g) < 0.3
    last = slot_rows(c.R, c.slots)[-1]
    dens = tail_dense_rows(c.R, last[1] - last[0], c.wrong, dense=0.5)
    wrong = torch.rand(shape, generator=g) < dens
    x = torch.where(t ^ wrong, LOGIT, -LOGIT).to(torch.float32)
    if c.family == 2:
        x[torch.rand(shape, generator=g) < 1.0 / 3] = 0.0
    w = None
    if c.weight != "none":
        vals = torch.tensor(c.wvals, dtype=torch.float32)
        wc = 1 if c.weight == "bcast" else c.C
        w = vals[torch.randint(0, len(vals), (c.N, wc, c.R), generator=g)].view(c.N, wc, *c.spatial)
    tt = {"float": torch.float32, "uint8": torch.uint8, "bool": torch.bool}[c.tdtype]
    return x.view(c.N, c.C, *c.spatial), t.to(tt).view(c.N, c.C, *c.spatial), w


def loss_quantum(c: LossCase) -> float:
    """the common divisor of every w * bce term of family 1"""
    wmin = min(v for v in c.wvals if v > 0) if c.weight != "none" else 1.0
    return LOGIT * wmin * min(1.0, 1.0 if c.pw is None else c.pw)


def loss_terms64(x, t, w, pw):
    """fp64 per-voxel (valid, w * bce, p) of the kernel's five sums; bce is analytic for |x| = 128 and ln 2 * lw at x = 0."""
    xd, td = x.double(), t.double()
    pwv = 1.0 if pw is None else float(pw)
    p = (xd > 0).double() + 0.5 * (xd == 0).double()
    bce = (xd > 0) * (1.0 - td) * LOGIT + (xd < 0) * td * (LOGIT * pwv) + (xd == 0) * (math.log(2.0) * (1.0 + (pwv - 1.0) * td))
    if w is None:
        return torch.ones_like(xd), bce, p
    wd = w.double().expand_as(xd)
    return (wd > 0).double(), wd * bce, p


def loss_sums64(x, t, w, pw, rows=None):
    """(N C, 5) fp64: sum w bce, #{w > 0}, sum p t, sum p, sum t over the valid voxels (rows: an optional (a, b) row range)."""
    valid, wb, p = loss_terms64(x, t, w, pw)
    td = t.double()
    N, C = x.shape[:2]
    cols = [valid * wb, valid, valid * p * td, valid * p, valid * td]
    out = []
    for col in cols:
        col = col.reshape(N * C, -1)
        if rows is not None:
            col = col[:, rows[0]:rows[1]]
        out.append(col.sum(1))
    return torch.stack(out, 1)


def loss_assert_caps(c: LossCase, x, t, w) -> torch.Tensor:
    """The exactness caps of one drawn case (fails on the CPU for an over-cap case); -> the exact sums (N C, 5)."""
    assert c.family == 1 or c.w_bce == 0.0, f"{c.name}: family 2 has an inexact bce term, w_bce must be 0"
    valid, wb, p = loss_terms64(x, t, w, c.pw)
    s = loss_sums64(x, t, w, c.pw)
    if c.family == 1:
        # one cap for the global numerator covers every (n, c) partial as well
        assert_exact_cap(float((valid * wb).abs().sum()), loss_quantum(c), what=c.name + " sum w bce")
        q = (wb / loss_quantum(c))
        assert bool((q == q.round()).all()), c.name + ": a w bce term is not a multiple of the quantum"
    if c.weight != "none":
        assert_exact_cap(float(s[:, 1].sum()), 1.0, what=c.name + " valid count")
    else:
        assert float(s[:, 1].max()) < EXACT_F32 and (c.N * c.C * c.R > EXACT_F32) == c.den_rounded
    qd = 0.5 if c.family == 2 else 1.0
    assert_exact_cap(float((s[:, 3] + s[:, 4]).max()) + c.sdr, qd, what=c.name + " dice denominator")
    assert_exact_cap(2.0 * float(s[:, 2].max()) + c.snr, qd, what=c.name + " dice numerator")
    return s


def loss_den64(c: LossCase, sums: torch.Tensor) -> float:
    """the bce denominator the kernel must report in parts[3]: the valid count (at least 1), or N C R rounded once to fp32"""
    if c.weight != "none":
        return max(float(sums[:, 1].sum()), 1.0)
    return float(torch.tensor(float(c.N * c.C), dtype=torch.float32) * torch.tensor(float(c.R), dtype=torch.float32))


def loss_ref64(sums: torch.Tensor, den: float, w_bce: float, w_dice: float, snr: float, sdr: float):
    """(loss, bce, dice) in fp64 from the exact sums"""
    bce = float(sums[:, 0].sum()) / den
    dice = float((1.0 - (2.0 * sums[:, 2] + snr) / (sums[:, 3] + sums[:, 4] + sdr)).mean())
    return w_bce * bce + w_dice * dice, bce, dice


def loss_grad64(x, t, w, sums, den, *, pw, w_bce, w_dice, snr, sdr, go=1.0, logistic=False):
    """fp64 dL/dlogits of w_bce bce + w_dice dice (the formula above bce_dice_bwd_kernel): exact sums in, masked voxels 0.
    logistic: p = sigmoid(x) in fp64 (the clamp-range group) instead of the exact {0, 1/2, 1} of the exact families."""
    xd, td = x.double(), t.double()
    pwv = 1.0 if pw is None else float(pw)
    p = torch.sigmoid(xd) if logistic else (xd > 0).double() + 0.5 * (xd == 0).double()
    N, C = x.shape[:2]
    view = (N, C) + (1,) * (x.dim() - 2)
    sums = sums.to(xd.device)
    I2 = (2.0 * sums[:, 2] + snr).view(view)
    Dn = (sums[:, 3] + sums[:, 4] + sdr).view(view)
    gb = (go * w_bce / den) * (p * (1.0 + (pwv - 1.0) * td) - pwv * td)
    gd = (go * w_dice / (N * C)) * (I2 - 2.0 * td * Dn) / (Dn * Dn) * p * (1.0 - p)
    if w is None:
        return gb + gd
    wd = w.double().expand_as(xd)
    return torch.where(wd > 0, wd * gb + gd, torch.zeros_like(gb))


def bce_dice_ref64(x, t, w, *, pw, w_bce, w_dice, snr, sdr, clamp_min=-20.0):
    """training/module.py's weighted_bce_with_logits + dice_loss_sigmoid on doubles (those functions cast to fp32, so their formulas
    are restated here; the host test holds the restatement to them).  The Dice term sees a weight map the way the module feeds it:
    through _mask_for_unweighted_loss (invalid voxels: logit clamp_min, target 0)."""
    xd, td = x.double(), t.double()
    pwt = None if pw is None else torch.as_tensor([float(pw)], dtype=torch.float64, device=xd.device)
    bce = F.binary_cross_entropy_with_logits(xd, td, pos_weight=pwt, reduction="none")
    if w is None:
        b = bce.mean()
        xm, tm = xd, td
    else:
        wd = w.double().expand_as(bce)
        valid = wd > 0
        b = (bce * wd * valid).sum() / valid.sum().clamp_min(1)
        xm, tm = xd.masked_fill(~valid, float(clamp_min)), td * valid
    p = torch.sigmoid(xm)
    dims = tuple(range(2, p.dim()))
    dice = (1.0 - (2.0 * (p * tm).sum(dims) + snr) / (p.sum(dims) + tm.sum(dims) + sdr)).mean()
    return w_bce * b + w_dice * dice


def clamp_range_operands(kind: str, shape, seed: int):
    """The clamp-range group (checked against fp64, not exactly): logits from the clamp values and their neighbourhood ('grid') or
    uniform in [-20, 20] ('uniform'), soft targets in [0, 1], a continuous weight map in [0, 2] with a zero region."""
    g = _gen(seed)
    if kind == "grid":
        vals = torch.tensor([-20.0, -19.99, -10.0, -1.0, -1e-3, 0.0, 1e-3, 1.0, 10.0, 19.99, 20.0])
        x = vals[torch.randint(0, len(vals), shape, generator=g)]
    else:
        x = torch.rand(shape, generator=g) * 40.0 - 20.0
    t = torch.rand(shape, generator=g)
    w = torch.rand((shape[0], 1, *shape[2:]), generator=g) * 2.0
    w[:, :, : max(1, shape[2] // 4)] = 0.0
    return x, t, w


# ---------------------------------------------------------------------------------------------------------------- optimizer
BOUNDARY_LENGTHS = (1, 4095, 4096, 4097, 8191, 8192, 8193, 3 * 4096 + 1)


def model_shapes(size: str = "S"):
    """parameter shapes of build_model's MedNeXt (size 'S': the Lucchi++ tutorial model; 'L': the MitoEM one), built on the meta
    device: no storage, no forward"""
    from types import SimpleNamespace as NS

    from pytorch_connectomics_amd.models import build_model
    cfg = NS(model=NS(arch=NS(type="mednext"), in_channels=1, out_channels=1, mednext=NS(size=size, kernel_size=3),
                      loss=NS(deep_supervision=False), heads=None, primary_head=None))
    with torch.device("meta"):
        model = build_model(cfg)
    return [tuple(p.shape) for p in model.parameters()]


def ternary_grad(shape, density: float, seed: int, scale: float = 1.0) -> torch.Tensor:
    from exact_reduction_cases import ternary
    return ternary(tuple(shape) if len(shape) else (1,), density, seed, scale=scale, dtype=torch.float32).reshape(shape)


def probe_grad(numel: int, kind: str) -> torch.Tensor:
    """zero everywhere except the last element ('last') or the first and last element of every chunk ('chunk_ends'): sum g^2 is a
    small integer, one lost element a whole unit of it"""
    g = torch.zeros(numel)
    if kind == "last":
        g[-1] = 1.0
    else:
        for c in range(opt_chunks(numel)):
            g[c * OPT_CHUNK] = 1.0
            g[min(numel, (c + 1) * OPT_CHUNK) - 1] = 1.0
    return g


def f32(v: float) -> float:
    return float(torch.tensor(float(v), dtype=torch.float32))


def adamw_row(lr, betas, eps, wd, t: int, ema_d: float, rounded: bool = True):
    """the scalar row FusedAdamW.step hands the kernel for step count t: (lr, b1, b2, eps, wd, 1 - b1^t, sqrt(1 - b2^t), d), formed in
    double and (rounded) stored as fp32"""
    b1, b2 = betas
    row = [lr, b1, b2, eps, wd, 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t), ema_d]
    return [f32(v) for v in row] if rounded else [float(v) for v in row]


def adamw_ref64(p, m, v, g, coef: float, row, ema=None):
    """One step of the documented update in fp64 from fp32 state: g c; p (1 - lr wd); m' = b1 m + (1 - b1) g c;
    v' = b2 v + (1 - b2) (g c)^2; p' = p (1 - lr wd) - (lr / bc1) m' / (sqrt(v') / bc2s + eps); ema' = d ema + (1 - d) p'.
    -> dict of (value, bound) per quantity; the bounds are derived in the module docstring."""
    lr, b1, b2, eps, wd, bc1, bc2s, d = row
    p, m, v, g = p.double(), m.double(), v.double(), g.double()
    gc = g * coef
    mn = b1 * m + (1.0 - b1) * gc
    vn = b2 * v + (1.0 - b2) * gc * gc
    M = (b1 * m).abs() + ((1.0 - b1) * gc).abs()
    den = vn.sqrt() / bc2s + eps
    step = lr / bc1
    pn = p * (1.0 - lr * wd) - step * mn / den
    bp = gamma(4) * p.abs() + gamma(25) * step * M / den + F32_MIN_NORMAL
    out = {"m": (mn, gamma(3) * M + F32_MIN_NORMAL), "v": (vn, gamma(5) * vn + F32_MIN_NORMAL), "p": (pn, bp)}
    if ema is not None:
        e = ema.double()
        out["ema"] = (d * e + (1.0 - d) * pn, gamma(3) * ((d * e).abs() + ((1.0 - d) * pn).abs()) + (1.0 - d) * bp + F32_MIN_NORMAL)
    return out


# ---------------------------------------------------------------------------------------------------------------- clDice
def blobs(shape, seed: int, density: float = 0.5, k: int = 7) -> torch.Tensor:
    """Binary {0, 1} fp32 volumes (N, C, *spatial) with structures several voxels thick (smoothed noise, thresholded at its
    `density` quantile per volume), so that the later erosion levels of the soft skeleton are not empty, as they are for white noise."""
    g = _gen(seed)
    r = torch.rand(shape, generator=g)
    nd = len(shape) - 2
    pool = F.avg_pool3d if nd == 3 else F.avg_pool2d
    for _ in range(2):
        r = pool(r, k, stride=1, padding=k // 2, count_include_pad=False)
    flat = r.reshape(shape[0] * shape[1], -1)
    thr = flat.kthvalue(max(1, int(flat.shape[1] * (1.0 - density))), dim=1).values
    return (flat > thr[:, None]).float().view(shape)


def cldice_weight(shape, seed: int) -> torch.Tensor:
    vals = torch.tensor([0.0, 0.5, 1.0, 2.0])
    return vals[torch.randint(0, 4, shape, generator=_gen(seed))]


CLDICE_SUM_CASES = (   # (name, shape, iteration counts)
    ("w112", (2, 1, 112, 112, 112), (3, 10)),
    ("plane1024x768", (2, 1, 1024, 768), (3, 10)),
    ("odd33x47x41", (2, 2, 33, 47, 41), (3, 10)),         # 63 591 voxels: 63 tiles, the last one 103 voxels
)


def cldice_sums64(skel, other, weight):
    """(N, C, 2) fp64: sum (s w)(other w), sum s w"""
    s, o = skel.double(), other.double()
    w = torch.ones_like(s) if weight is None else weight.double()
    dims = tuple(range(2, s.dim()))
    return torch.stack([((s * w) * (o * w)).sum(dims), (s * w).sum(dims)], -1)

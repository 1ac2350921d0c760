"""Exact-arithmetic cases for the norm / activation / pool chain of the dense-conv models (csrc/norm_pool_kernels.hip and the
backward half in csrc/rsunet_train_kernels.hip): operands, fp64 references, fp32 CPU restatements of the kernel formulas (with
seeded defects), slot-count mirrors and the case tables.  Plain module (no tests): test_gpu_norm_act_exact.py runs the cases on the
kernels, test_host_norm_act_exact_cases.py proves on the CPU that the cases do what they claim.

What is exact.  x and da are ternary ({-s, 0, s}, s a power of two), the norm affine comes from exact_affine (a in {+-1/2, +-1, +-2},
b in {-2 .. 2}), mean in {-1, 0, 1}, rstd in {1/4, 1/2, 1, 2}, gamma in {+-1/2, +-1, +-2}, M1 / M2 multiples of 1/8, the leaky / PReLU
slope is 1/4.  Then t = a x + b, act'(t), dt = da act'(t), dp = da min(t, 0), xhat = (x - mean) rstd, every term of sum dt,
sum dt xhat and sum dp, and dx = rstd (gamma dt - M1 - xhat M2) are dyadic numbers of a few bits: exact in fp32 and (the stored
ones) in bf16, in any order of evaluation, with or without fma contraction; the sums stay below 2^24 quanta (checked per case).  The
correct result is the fp64 result bit for bit (bf16 storage: bf16 of it).  dt and dp are compared as bit patterns, so that the sign of
a zero (t == -0.0, da < 0) is part of the check; sums and dx are compared by value.

What is bounded, and by what (u = 2^-24, all against fp64 of the exact inputs, never against a kernel's output).

  norm_finalize_groups / bn_train_finalize, from integer slot statistics (t1 = sum x, t2 = sum x^2 exact in fp32, cnt exact):
    mean = fl(t1 / cnt)                                   |d mean| <= u |mean|
    q    = fl(t2 / cnt), var = fl(q - mean^2)              |d var|  <= u (q + 3 mean^2 + var)   (q, the square, its two factors, the
                                                            subtraction; an fma only removes a term) =: e_var var.  The cancellation
                                                            factor q / var is at most 1 + mean^2 / var <= 5 for |mean| <= 1, var >= 1/4
    v    = fl(var + eps)                                   relative e_v = e_var + u
    rstd = rsqrtf(v), one Newton step r (1.5 - 0.5 v r r): the hardware reciprocal square root is good to 1 ulp (2 u); the step squares
           that error (4 u^2: nothing) and adds the roundings of its own evaluation: 0.5 v r r carries 2 u of 1/2, the subtraction
           from 1.5 one more u of 1, the product with r one more: 3 u.  Together with the inherited half of e_v:
                                                            e_r = e_v / 2 + 3 u + u (slack for second-order terms)
    a    = fl(gamma rstd)                                  e_a = e_r + u
    b    = fl(beta - mean a)                               |d b| <= |mean a| (e_a + 2 u) + u |b|
  The padded channels carry exactly 0 in all four.

  norm_bwd_means: M = (sum_j s_j gamma_j) * fl(1 / (rows cpg)): the sum is exact (dyadic s, gamma a power of two); where rows cpg is a
  power of two so are the reciprocal and the product (M exact), otherwise two roundings: |d M| <= (2 u + u^2) |M|.

  BatchNorm running buffers: var_b = fl(fl(1 / fl(rstd rstd)) - eps) recovered from rstd (relative error e_r, or 0 where rstd is an
  input): |d var_b| <= (var + eps) (2 e_r + 2 u) + u var; unbiased: times fl(cnt / (cnt - 1)): 2 u more; the blend
  (1 - m) old + m new with m = fp32(momentum): |m - momentum| <= u momentum, fl(1 - m) u, two products and the sum (or an fma):
    |d rvar| <= m |d var_u| + 3 u (|old| + |new|)     and the same with d mean = u |mean| for the running mean.

  ELU / sigmoid / tanh: __expf and tanhf have no stated bound in the installed ROCm headers (__clang_hip_math.h defines __expf(x) as
  exp2 of fl(log2(e) x) on the hardware exponential and says nothing of its error), so the margins are measured once on the GPU over
  every bf16 value in [-88, 8] and doubled (profiles/norm_act_exact_probe.txt); INTRINSIC_MARGIN holds the doubled values."""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from exact_reduction_cases import EXACT_F32, U32, colstats_slots, exact_affine, slot_rows, tail_dense_rows, ternary  # noqa: F401

ACT_NONE, ACT_SIGMOID, ACT_TANH, ACT_RELU, ACT_LEAKY, ACT_ELU = 0, 1, 2, 5, 6, 7       # pytorch_connectomics_amd/_native.py
SLOPE = 0.25
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}
EXACT_ACTS = (("none", ACT_NONE, 0.0, False), ("relu", ACT_RELU, 0.0, False), ("leaky", ACT_LEAKY, SLOPE, False),
              ("prelu", ACT_LEAKY, SLOPE, True))

# 2 x the largest |kernel - fp64| over every bf16 argument in [-88, 8], fp32 storage (profiles/norm_act_exact_probe.txt):
# affine_act ELU / sigmoid / tanh outputs and the ELU derivative of act_bwd (da = 1).
INTRINSIC_MARGIN = {"elu": 2 * 5.7009e-08, "sigmoid": 2 * 8.5235e-08, "tanh": 2 * 5.5371e-08, "elu_der": 2 * 4.1959e-08}
# rel-L2 of the fp32 CPU restatement of the chain (norm -> ELU, forward and backward) against fp64 autograd, same seeds, worst over
# the three norm kinds (profiles/norm_act_exact_probe.txt); the chain cases allow 2 x these
CHAIN_RESTATED_REL_L2 = {"f32": {"out": 5.1119e-08, "dx": 7.4249e-08, "dgamma": 3.8340e-07, "dbeta": 3.2539e-07},
                         "bf16": {"out": 1.6438e-03, "dx": 1.8994e-03, "dgamma": 7.8129e-04, "dbeta": 7.1668e-04}}


def epv(dtype) -> int:
    return 8 if dtype == torch.bfloat16 else 4


def bits(t: torch.Tensor) -> torch.Tensor:
    """the bit patterns of a bf16 / fp32 tensor (distinguishes -0.0 from 0.0)"""
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---------------------------------------------------------------------------------------------------------------- slot mirrors
def act_norm_slots(rows: int, C: int, dtype) -> int:
    """rsunet_train_kernels.hip act_norm_slots: >= 16 rows per row lane, at most colstats_slots(rows)"""
    chunks = C // epv(dtype)
    cw = min(chunks, 256)
    rl = 256 // cw
    return max(1, min(colstats_slots(rows), rows // (rl * 16)))


def row_lanes(C: int, dtype):
    """(Cw, RL, idle threads) of the first channel window of the two fused kernels"""
    cw = min(C // epv(dtype), 256)
    return cw, 256 // cw, 256 - cw * (256 // cw)


# ---------------------------------------------------------------------------------------------------------------- operands
def signed_ternary(shape, seed: int, *, scale=1.0, dtype=torch.bfloat16, device="cpu", density=0.5, row_density=None):
    """ternary values whose zeros carry a seeded sign (-0.0 as well as 0.0)"""
    t = ternary(shape, density, seed, scale=scale, dtype=torch.float32, device=device, row_density=row_density)
    g = torch.Generator(device=device).manual_seed(int(seed) + 7919)
    sgn = (torch.rand(shape, generator=g, device=device) < 0.5).float() * 2.0 - 1.0
    return (t * sgn).to(dtype)


def affine_negzero(N: int, C: int, seed: int) -> torch.Tensor:
    """exact_affine with half of its b == 0 entries turned into -0.0: a x + b is then -0.0 for x = -+0.0 (sign of -a)"""
    ab = exact_affine(N, C, seed)
    g = torch.Generator().manual_seed(int(seed) + 31)
    flip = (torch.rand((N, C), generator=g) < 0.5) & (ab[:, 1] == 0)
    ab[:, 1] = torch.where(flip, torch.tensor(-0.0), ab[:, 1])
    ab[:, 0, 0], ab[:, 1, 0] = 1.0, -0.0                     # whatever the draw: channel 0 maps x = -0.0 to t = -0.0, 0.0 to 0.0
    if C > 1:
        ab[:, 0, 1], ab[:, 1, 1] = -2.0, -0.0                # ... and channel 1 maps x = 0.0 to t = -0.0
    return ab.contiguous()


def _pick(vals, shape, g):
    v = torch.tensor(vals, dtype=torch.float32)
    return v[torch.randint(0, len(vals), shape, generator=g)]


def exact_mean_rstd(N: int, C: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(int(seed))
    return torch.stack([_pick([-1.0, 0.0, 1.0], (N, C), g), _pick([0.25, 0.5, 1.0, 2.0], (N, C), g)], 1).contiguous()


def exact_gamma(C: int, seed: int) -> torch.Tensor:
    return _pick([0.5, -0.5, 1.0, -1.0, 2.0, -2.0], (C,), torch.Generator().manual_seed(int(seed)))


def exact_M(N: int, C: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(int(seed))
    return (torch.randint(-8, 9, (N, 2, C), generator=g).float() / 8.0).contiguous()


@dataclass(frozen=True)
class FusedCase:
    """one shape of act_norm_bwd_stats / act_norm_bwd_apply; gamma_short: entries of the short gamma form (0: none for this shape)"""
    storage: str
    N: int
    rows: int
    C: int
    gamma_short: int
    what: str

    @property
    def dtype(self):
        return DTYPES[self.storage]

    @property
    def slots(self) -> int:
        return act_norm_slots(self.rows, self.C, self.dtype)

    @property
    def name(self) -> str:
        return f"{self.storage}-N{self.N}-rows{self.rows}-C{self.C}-slots{self.slots}"


FUSED_CASES = [
    FusedCase("bf16", 2, 9216 + 37, 8, 0, "Cw = 1, RL = 256, ragged last slot"),
    FusedCase("bf16", 2, 2 * 1360 + 11, 24, 18, "Cw = 3, RL = 85: one idle lane"),
    FusedCase("bf16", 1, 3 * 816 + 5, 40, 36, "Cw = 5, RL = 51: one idle lane"),
    FusedCase("bf16", 3, 1200, 64, 0, "Cw = 8, three samples"),
    FusedCase("f32", 2, 2 * 816 + 3, 20, 18, "Cw = 5 in fp32"),
    FusedCase("f32", 1, 2 * 448 + 9, 36, 0, "Cw = 9, RL = 28: four idle lanes"),
]
WINDOW_CASE = FusedCase("bf16", 2, 128, 2056, 0, "257 chunks: a second channel window with Cw = 1, RL = 256")


def fused_operands(c: FusedCase, seed: int, *, with_ab: bool = True, device="cpu") -> dict:
    """x, da (N, rows, C) in the storage type, ab / mr / M fp32, gamma (C).  The last rows of every sample are dense (the last slot
    carries signal), the rest sparse."""
    tail = max(8, c.rows - slot_rows(c.rows, c.slots)[-1][0]) if c.slots > 1 else 8
    dens = tail_dense_rows(c.rows, min(tail, 64), 0.25).repeat(c.N)
    shape = (c.N, c.rows, c.C)
    x = signed_ternary(shape, seed, dtype=c.dtype, device=device, row_density=dens)
    da = signed_ternary(shape, seed + 1, scale=0.5, dtype=c.dtype, device=device, row_density=dens)
    return dict(x=x, da=da, ab=affine_negzero(c.N, c.C, seed + 2).to(device) if with_ab else None,
                mr=exact_mean_rstd(c.N, c.C, seed + 3).to(device), M=exact_M(c.N, c.C, seed + 4).to(device),
                gamma=exact_gamma(c.C, seed + 5).to(device))


# ---------------------------------------------------------------------------------------------------------------- fp64 references
def _bc(v: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """(N, C) coefficients broadcast over x (N, ..., C)"""
    return v.double().view(v.shape[0], *([1] * (x.dim() - 2)), v.shape[-1])


def ref_t(x, ab, storage=None) -> torch.Tensor:
    """t = a x + b in fp64 (x itself without ab), rounded to `storage` where the backward kernels round it"""
    t = x.double()
    if ab is not None:
        t = t * _bc(ab[:, 0], x) + _bc(ab[:, 1], x)
        if storage is not None:
            t = t.to(storage).double()
    return t


def act64(t, act: int, prm: float):
    if act == ACT_RELU:
        return torch.where(t > 0, t, torch.zeros_like(t))
    if act == ACT_LEAKY:
        return torch.where(t > 0, t, t * prm)
    if act == ACT_ELU:
        return torch.where(t > 0, t, prm * torch.expm1(t))
    if act == ACT_SIGMOID:
        return torch.sigmoid(t)
    if act == ACT_TANH:
        return torch.tanh(t)
    return t


def act_der64(t, act: int, prm: float):
    one = torch.ones_like(t)
    if act == ACT_RELU:
        return torch.where(t > 0, one, torch.zeros_like(t))
    if act == ACT_LEAKY:
        return torch.where(t > 0, one, one * prm)
    if act == ACT_ELU:
        return torch.where(t > 0, one, prm * torch.exp(t))
    return one


def ref_affine_act(x, ab, act, prm):
    return act64(ref_t(x, ab), act, prm)


def ref_act_bwd(da, x, ab, act, prm):
    """(dt, dp) in fp64: dt = da act'(t), dp = da min(t, 0) with +0.0 wherever t is not below zero (torch's PReLU backward)"""
    t = ref_t(x, ab, x.dtype)
    d = da.double()
    return d * act_der64(t, act, prm), torch.where(t < 0, d * t, torch.zeros_like(t))


def ref_xhat(x, mr):
    return (x.double() - _bc(mr[:, 0], x)) * _bc(mr[:, 1], x)


def ref_bwd_stats(da, x, ab, mr, act, prm, rows=None):
    """s (N, 2, C) = (sum dt, sum dt xhat), p (N, C) = sum dp over the rows [rows[0], rows[1]) of every sample (all by default)"""
    dt, dp = ref_act_bwd(da, x, ab, act, prm)
    dt, dp = dt.to(x.dtype).double(), dp.to(x.dtype).double()
    xh = ref_xhat(x, mr)
    N, C = x.shape[0], x.shape[-1]
    dt, dp, xh = (v.reshape(N, -1, C) for v in (dt, dp, xh))
    if rows is not None:
        dt, dp, xh = (v[:, rows[0]:rows[1]] for v in (dt, dp, xh))
    return torch.stack([dt.sum(1), (dt * xh).sum(1)], 1), dp.sum(1)


def zero_extended(gamma, C: int):
    if gamma is None:
        return None
    return F.pad(gamma, (0, C - gamma.numel())) if gamma.numel() < C else gamma


def ref_bwd_apply(da, x, ab, mr, gamma, M, act, prm):
    """dx = rstd (gamma dt - M1 - xhat M2) in fp64, gamma zero-extended to the channels of x"""
    dt = ref_act_bwd(da, x, ab, act, prm)[0].to(x.dtype).double()
    g = torch.ones(x.shape[-1], dtype=torch.float64, device=x.device) if gamma is None else zero_extended(gamma, x.shape[-1]).double()
    return _bc(mr[:, 1], x) * (g * dt - _bc(M[:, 0], x) - ref_xhat(x, mr) * _bc(M[:, 1], x))


def fused_caps(c: FusedCase, o: dict) -> dict:
    """sum |term| of the largest output of each sum, in quanta: dt multiples of 1/8 (da 1/2, slope 1/4), xhat of 1/4, t of 1/2"""
    t = ref_t(o["x"], o["ab"], o["x"].dtype)
    d = o["da"].double().abs()
    xh = ref_xhat(o["x"], o["mr"]).abs()
    return {"sum dt": float(d.sum(1).max()) * 8, "sum dt xhat": float((d * xh).sum(1).max()) * 32,
            "sum dp": float((d * t.abs()).sum(1).max()) * 4}


# ---------------------------------------------------------------------------------------------------------------- fp32 restatements
def _st(v: torch.Tensor, dtype) -> torch.Tensor:
    """round an fp32 value to the storage type and back (from_f32 / to_f32)"""
    return v.to(dtype).float()


def _sample_index(x: torch.Tensor, vec: int, defect):
    """sample index per element of x (N, rows, C) as the vector kernels compute it: chunk q / (rows C / VEC); the defect divides by
    rows C (a chunk index taken for an element index)"""
    N, rows, C = x.shape
    q = torch.arange(x.numel() // vec).repeat_interleave(vec).view(N, rows, C)
    per = rows * C if defect == "sample_index" else rows * (C // vec)
    return (q // per).clamp_(max=N - 1)


def restate_t(x, ab, *, vec: int = 1, defect=None, round_to=None):
    t = x.float()
    if ab is not None:
        n = _sample_index(x, vec, defect)
        c = torch.arange(x.shape[-1]).view(1, 1, -1).expand_as(n)
        t = torch.addcmul(ab[n, 1, c], t, ab[n, 0, c])
        if round_to is not None:
            t = _st(t, round_to)
    return t


def restate_affine_act(x, ab, act, prm, *, vec: int = 1, defect=None):
    """affine_act_kernel / affine_act_vec_kernel on x (N, rows, C)"""
    v = restate_t(x, ab, vec=vec, defect=defect)
    pos = (v >= 0) if defect == "kink_ge" else (v > 0)
    if act == ACT_RELU:
        v = torch.where(pos, v, torch.zeros_like(v))
    elif act == ACT_LEAKY:
        v = torch.where(pos, v, v * prm)
    elif act == ACT_ELU:
        v = torch.where(pos, v, prm * (torch.exp(v) - 1.0))
    elif act == ACT_SIGMOID:
        v = 1.0 / (1.0 + torch.exp(-v))
    elif act == ACT_TANH:
        v = torch.tanh(v)
    return v.to(x.dtype)


def restate_act_bwd(da, x, ab, act, prm, *, vec: int = 1, defect=None):
    """act_bwd_kernel / act_bwd_vec_kernel / act_dt_vec: (dt, dp) in the storage type"""
    t = restate_t(x, ab, vec=vec, defect=defect, round_to=x.dtype)
    d = da.float()
    pos = (t >= 0) if defect == "kink_ge" else (t > 0)
    one = torch.ones_like(t)
    if act == ACT_RELU:
        der = torch.where(pos, one, torch.zeros_like(t))
    elif act == ACT_LEAKY:
        der = torch.where(pos, one, one * prm)
    elif act == ACT_ELU:
        der = torch.where(pos, one, prm * torch.exp(t))
    else:
        der = one
    neg = (t <= 0) if defect == "dp_le" else (t < 0)
    return (d * der).to(x.dtype), torch.where(neg, d * t, torch.zeros_like(t)).to(x.dtype)


def restate_bwd_stats(da, x, ab, mr, act, prm, slots: int, *, defect=None):
    """act_norm_bwd_stats_kernel + reduce_slots: per-slot fp32 sums over the ceil-divided row split, then the slots in order.
    defects: last_slot (dropped), slot_off_by_one (every slot but the first starts one row late), sample_index, kink_ge, dp_le"""
    dt, dp = restate_act_bwd(da, x, ab, act, prm, vec=epv(x.dtype), defect=defect)
    dt, dp = dt.float(), dp.float()
    xh = (x.float() - mr[:, 0].unsqueeze(1)) * mr[:, 1].unsqueeze(1)
    N, rows, C = x.shape
    s = torch.zeros(N, 2, C)
    p = torch.zeros(N, C)
    sl = slot_rows(rows, slots)
    for i, (a, b) in enumerate(sl):
        if defect == "last_slot" and i == len(sl) - 1 and i > 0:
            continue
        if defect == "slot_off_by_one" and i > 0:
            a += 1
        s[:, 0] += dt[:, a:b].sum(1)
        s[:, 1] += (dt[:, a:b] * xh[:, a:b]).sum(1)
        p += dp[:, a:b].sum(1)
    return s, p


def restate_bwd_apply(da, x, ab, mr, gamma, M, act, prm, slots: int, *, defect=None):
    """act_norm_bwd_apply_kernel.  defects: gamma_tail (a short gamma continued with ones instead of zeros), last_slot (its rows
    never written: left at the fill value 0), slot_off_by_one, sample_index, kink_ge"""
    dt = restate_act_bwd(da, x, ab, act, prm, vec=epv(x.dtype), defect=defect)[0].float()
    N, rows, C = x.shape
    if gamma is None:
        g = torch.ones(C)
    elif gamma.numel() < C:
        g = F.pad(gamma, (0, C - gamma.numel()), value=1.0 if defect == "gamma_tail" else 0.0)
    else:
        g = gamma
    xh = (x.float() - mr[:, 0].unsqueeze(1)) * mr[:, 1].unsqueeze(1)
    dx = mr[:, 1].unsqueeze(1) * (g * dt - M[:, 0].unsqueeze(1) - xh * M[:, 1].unsqueeze(1))
    sl = slot_rows(rows, slots)
    if defect == "last_slot" and len(sl) > 1:
        dx[:, sl[-1][0]:] = 0
    if defect == "slot_off_by_one":
        for a, _ in sl[1:]:
            dx[:, a] = 0
    return dx.to(x.dtype)


# ---------------------------------------------------------------------------------------------------------------- group algebra
@dataclass(frozen=True)
class GroupCase:
    groups: int        # 0: batch statistics
    cpg: int           # 0: C / groups
    C: int

    @property
    def width(self) -> int:
        return self.cpg if self.cpg > 0 else (self.C // self.groups if self.groups else 1)

    @property
    def c_real(self) -> int:
        return self.groups * self.width if self.groups else self.C

    @property
    def name(self) -> str:
        return f"g{self.groups}-cpg{self.cpg}-C{self.C}"


GROUP_CASES = [GroupCase(3, 6, 24), GroupCase(4, 9, 40), GroupCase(18, 1, 24), GroupCase(12, 2, 24), GroupCase(4, 0, 16),
               GroupCase(1, 0, 8), GroupCase(0, 0, 40)]
MEANS_ROWS = 4096
GROUP_N = 3


def means_exact(c: GroupCase, rows: int = MEANS_ROWS) -> bool:
    n = rows * c.width if c.groups else GROUP_N * rows
    return n & (n - 1) == 0


def means_operands(c: GroupCase, seed: int):
    """s (N, 2, C): multiples of 1/4 in [-64, 64] on every channel (the padded ones too: M must be 0 there whatever s holds);
    gamma (c_real) in {+-1/2, +-1, +-2}"""
    g = torch.Generator().manual_seed(int(seed))
    s = (torch.randint(-256, 257, (GROUP_N, 2, c.C), generator=g).float() / 4.0).contiguous()
    return s, exact_gamma(c.c_real, seed + 1)


def ref_means(s, gamma, c: GroupCase, rows: int):
    """fp64 (M, dgamma, dbeta, bound of M): bound 0 where rows cpg is a power of two, else (2 u + u^2) |M|"""
    N, _, C = s.shape
    sd = s.double()
    g = torch.ones(c.c_real, dtype=torch.float64) if gamma is None else gamma.double()
    M = torch.zeros_like(sd)
    if c.groups == 0:
        M[:] = (sd.sum(0) * g / (N * rows)).unsqueeze(0)
    else:
        w = c.width
        sg = (sd[:, :, :c.c_real] * g).view(N, 2, c.groups, w).sum(-1, keepdim=True) / (rows * w)
        M[:, :, :c.c_real] = sg.expand(N, 2, c.groups, w).reshape(N, 2, c.c_real)
    bound = torch.zeros_like(M) if means_exact(c, rows) else (2 * U32 + U32 * U32) * M.abs()
    return M, sd[:, 1].sum(0), sd[:, 0].sum(0), bound


def restate_means(s, gamma, c: GroupCase, rows: int, *, defect=None):
    """norm_bwd_means_kernel in fp32.  defects: group_shift (every group starts one channel late), pad_counted (cpg taken as
    C / groups: the padding joins the groups)"""
    N, _, C = s.shape
    M = torch.zeros_like(s)
    dg, db = s[:, 1].sum(0), s[:, 0].sum(0)
    if c.groups == 0:
        gm = torch.ones(C) if gamma is None else gamma
        inv = torch.tensor(1.0) / torch.tensor(float(N) * float(rows))
        M[:] = torch.stack([db * gm * inv, dg * gm * inv]).unsqueeze(0)
        return M, dg, db
    w = c.width
    if defect == "pad_counted":
        w = C // c.groups
    inv = torch.tensor(1.0) / torch.tensor(float(rows) * float(w))
    gfull = torch.ones(C) if gamma is None else F.pad(gamma, (0, C - gamma.numel()), value=1.0)
    off = 1 if defect == "group_shift" else 0
    for gi in range(c.groups):
        lo, hi = gi * w + off, min(C, (gi + 1) * w + off)
        acc = torch.zeros(N, 2)
        for j in range(lo, hi):
            acc = acc + s[:, :, j] * gfull[j]
        M[:, :, lo:hi] = (acc * inv).unsqueeze(-1)
    return M, dg, db


FINALIZE_SLOTS = (1, 7, 400, 1024)
STAT_ROWS_PER_SLOT = 64


def synthetic_stats(N: int, slots: int, C: int, c_real: int, seed: int) -> torch.Tensor:
    """integer-valued slot statistics (N, slots, 2, C) of STAT_ROWS_PER_SLOT rows per slot, zero on the padded channels: per
    (sample, channel) a mean in [-3/4, 3/4] and a variance in {1/2, 1, 2, 3} plus per-slot integer noise, so that every group has
    |mean| <= 1 and var in [1/4, 4] (asserted by the host checks); all sums stay far below 2^24"""
    L = STAT_ROWS_PER_SLOT
    g = torch.Generator().manual_seed(int(seed))
    m = _pick([-0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75], (N, 1, C), g)
    v = _pick([0.5, 1.0, 2.0, 3.0], (N, 1, C), g)
    s1 = L * m + torch.randint(-8, 9, (N, slots, C), generator=g).float()
    s2 = L * (v + m * m) + torch.randint(0, 16, (N, slots, C), generator=g).float()
    st = torch.stack([s1, s2], 2).round()
    st[..., c_real:] = 0
    return st.contiguous()


def general_gamma_beta(c_real: int, seed: int):
    g = torch.Generator().manual_seed(int(seed))
    return (torch.rand(c_real, generator=g) + 0.5).contiguous(), torch.randn(c_real, generator=g).contiguous()


def _finalize_bounds(mean, q, var, eps, gamma, beta):
    """the docstring's error model, elementwise in fp64 -> bounds of (a, b, mean, rstd) and the relative error e_r of rstd"""
    u = U32
    e_var = u * (q + 3 * mean * mean + var) / var
    e_r = 0.5 * (e_var + u) + 4 * u
    rstd = 1.0 / torch.sqrt(var + eps)
    a = gamma * rstd
    b = beta - mean * a
    e_a = e_r + u
    return dict(a=a.abs() * e_a, b=(mean * a).abs() * (e_a + 2 * u) + u * b.abs(), mean=u * mean.abs(), rstd=rstd * e_r, e_r=e_r)


def ref_finalize(stats, count: float, gamma, beta, eps: float, c: GroupCase):
    """fp64 (ab (N, 2, C), mr (N, 2, C), bounds dict of (N, C) tensors), zero on the padded channels"""
    N, slots, _, C = stats.shape
    w, G, cr = c.width, c.groups, c.c_real
    t = stats.double().sum(1)[:, :, :cr].view(N, 2, G, w).sum(-1)                  # (N, 2, G)
    cnt = count * w
    mean, q = t[:, 0] / cnt, t[:, 1] / cnt
    var = q - mean * mean
    ex = lambda v: v.unsqueeze(-1).expand(N, G, w).reshape(N, cr)                 # noqa: E731
    mean, q, var = ex(mean), ex(q), ex(var)
    g = torch.ones(cr, dtype=torch.float64) if gamma is None else gamma.double()
    bt = torch.zeros(cr, dtype=torch.float64) if beta is None else beta.double()
    bd = _finalize_bounds(mean, q, var, eps, g, bt)
    rstd = 1.0 / torch.sqrt(var + eps)
    a = g * rstd
    pad = lambda v: F.pad(v, (0, C - cr))                                         # noqa: E731
    ab = torch.stack([pad(a), pad(bt - mean * a)], 1)
    mr = torch.stack([pad(mean), pad(rstd)], 1)
    return ab, mr, {k: pad(v) for k, v in bd.items()}, dict(mean=mean, var=var)


def restate_finalize(stats, count: float, gamma, beta, eps: float, c: GroupCase, *, defect=None):
    """norm_finalize_groups_kernel in fp32 (sums of the integer statistics are exact in any order).  defects: last_slot,
    group_shift, pad_counted"""
    N, slots, _, C = stats.shape
    w, G = c.width, c.groups
    if defect == "pad_counted":
        w = C // G
    st = stats[:, :-1] if (defect == "last_slot" and slots > 1) else stats
    tot = st.sum(1)                                                                # (N, 2, C) fp32, exact
    ab, mr = torch.zeros(N, 2, C), torch.zeros(N, 2, C)
    off = 1 if defect == "group_shift" else 0
    cnt = torch.tensor(float(count) * float(w))
    gfull = torch.ones(C) if gamma is None else F.pad(gamma, (0, C - gamma.numel()), value=1.0)
    bfull = torch.zeros(C) if beta is None else F.pad(beta, (0, C - beta.numel()))
    for gi in range(G):
        lo, hi = gi * w + off, min(C, (gi + 1) * w + off)
        t1, t2 = tot[:, 0, lo:hi].sum(-1), tot[:, 1, lo:hi].sum(-1)
        mean = t1 / cnt
        var = torch.clamp(t2 / cnt - mean * mean, min=0.0)
        v = var + eps
        r = torch.rsqrt(v)
        r = r * (1.5 - 0.5 * v * r * r)
        a = gfull[lo:hi] * r.unsqueeze(-1)
        ab[:, 0, lo:hi] = a
        ab[:, 1, lo:hi] = bfull[lo:hi] - mean.unsqueeze(-1) * a
        mr[:, 0, lo:hi] = mean.unsqueeze(-1)
        mr[:, 1, lo:hi] = r.unsqueeze(-1)
    return ab, mr


# ---------------------------------------------------------------------------------------------------------------- BatchNorm
BN_CASES = [(18, 24), (36, 40), (16, 16)]          # (C_real, C)
BN_SLOTS_TOTAL = (3, 300)
BN_MOMENTA = (0.1, 0.0)
BN_EPS = 1e-5


def bn_old_running(c_real: int, seed: int):
    g = torch.Generator().manual_seed(int(seed))
    return torch.randn(c_real, generator=g).contiguous(), (torch.rand(c_real, generator=g) + 0.5).contiguous()


def ref_bn(stats, count: float, gamma, beta, eps: float, momentum: float, c_real: int, rmean, rvar):
    """fp64 BatchNorm (training): (a, b, mean, rstd) (C) zero-padded, the new running buffers (c_real) as nn.BatchNorm3d forms them
    (unbiased variance, momentum blend), and their bounds"""
    C = stats.shape[-1]
    t = stats.double().reshape(-1, 2, C).sum(0)[:, :c_real]
    mean, q = t[0] / count, t[1] / count
    var = q - mean * mean
    g = torch.ones(c_real, dtype=torch.float64) if gamma is None else gamma.double()
    bt = torch.zeros(c_real, dtype=torch.float64) if beta is None else beta.double()
    bd = _finalize_bounds(mean, q, var, eps, g, bt)
    rstd = 1.0 / torch.sqrt(var + eps)
    a = g * rstd
    pad = lambda v: F.pad(v, (0, C - c_real))                                     # noqa: E731
    out = dict(a=pad(a), b=pad(bt - mean * a), mean=pad(mean), rstd=pad(rstd), bounds={k: pad(v) for k, v in bd.items()},
               premise=dict(mean=mean, var=var))
    if rmean is not None:
        out.update(ref_running(mean, var, bd["e_r"], U32 * mean.abs(), count, eps, momentum, rmean, rvar))
    return out


def ref_running(mean, var, e_r, d_mean, count: float, eps: float, momentum: float, rmean, rvar):
    """the running-buffer blend in fp64 and its bound (docstring); e_r: relative error of the rstd the variance is recovered from"""
    u = U32
    unb = count / (count - 1.0) if count > 1 else 1.0
    new_var = var * unb
    d_var = ((var + eps) * (2 * e_r + 2 * u) + u * var) * unb + 2 * u * new_var
    om, ov = rmean.double(), rvar.double()
    return dict(rmean=(1 - momentum) * om + momentum * mean, rvar=(1 - momentum) * ov + momentum * new_var,
                rmean_bound=momentum * d_mean + 3 * u * (om.abs() + mean.abs()),
                rvar_bound=momentum * d_var + 3 * u * (ov.abs() + new_var.abs()))


def restate_bn(stats, count: float, gamma, beta, eps: float, momentum: float, c_real: int, rmean, rvar, *, defect=None):
    """bn_train_finalize_kernel in fp32 -> (a, b, mean, rstd (C), rmean, rvar (c_real) or None).  defects: last_slot, pad_counted
    (count taken over C / c_real times as many elements: the padding's zeros join the statistics)"""
    C = stats.shape[-1]
    st = stats.reshape(-1, 2, C)
    if defect == "last_slot" and st.shape[0] > 1:
        st = st[:-1]
    t = st.sum(0)[:, :c_real]
    cnt = torch.tensor(float(count) * (C / c_real if defect == "pad_counted" else 1.0))
    mean = t[0] / cnt
    var = torch.clamp(t[1] / cnt - mean * mean, min=0.0)
    v = var + eps
    r = torch.rsqrt(v)
    r = r * (1.5 - 0.5 * v * r * r)
    a = (torch.ones(c_real) if gamma is None else gamma) * r
    b = (torch.zeros(c_real) if beta is None else beta) - mean * a
    pad = lambda z: F.pad(z, (0, C - c_real))                                     # noqa: E731
    nm = nv = None
    if rmean is not None:
        nm, nv = restate_running(mean, r, cnt, eps, momentum, rmean, rvar)
    return pad(a), pad(b), pad(mean), pad(r), nm, nv


def restate_running(mean, rstd, cnt, eps: float, momentum: float, rmean, rvar):
    """bn_update_running_kernel / the tail of bn_train_finalize_kernel in fp32"""
    cnt = torch.as_tensor(cnt, dtype=torch.float32)
    m = torch.tensor(momentum, dtype=torch.float32)
    var = torch.clamp(1.0 / (rstd * rstd) - eps, min=0.0) * (cnt / torch.clamp(cnt - 1.0, min=1.0) if cnt > 1 else 1.0)
    return (1.0 - m) * rmean + m * mean, (1.0 - m) * rvar + m * var


# ---------------------------------------------------------------------------------------------------------------- elementwise cases
ELEMENTWISE_SHAPES = [("bf16", (2, 3, 5, 7, 24)), ("bf16", (2, 3, 5, 7, 40)), ("bf16", (2, 3, 5, 7, 64)), ("bf16", (3, 3, 5, 7, 24)),
                      ("bf16", (2, 3, 5, 7, 5)), ("bf16", (2, 3, 5, 7, 18)),
                      ("f32", (2, 3, 5, 7, 20)), ("f32", (2, 3, 5, 7, 36)), ("f32", (3, 3, 5, 7, 36)),
                      ("f32", (2, 3, 5, 7, 5)), ("f32", (2, 3, 5, 7, 18))]
GRID_CAP = 16384 * 256
GRID_CAP_VEC_SHAPE = (2, 129, 128, 128, 8)          # bf16: 4 227 072 chunks of 8
GRID_CAP_SCALAR_SHAPE = (2, 7, 173, 347, 5)         # 4 202 170 elements, scalar form only


def has_vec(C: int, dtype) -> bool:
    return C % epv(dtype) == 0


def elementwise_operands(storage: str, shape, seed: int, *, with_ab: bool, device="cpu"):
    dt = DTYPES[storage]
    x = signed_ternary(shape, seed, dtype=dt, device=device)
    da = signed_ternary(shape, seed + 1, scale=0.5, dtype=dt, device=device)
    ab = affine_negzero(shape[0], shape[-1], seed + 2).to(device) if with_ab else None
    return x, da, ab


def smooth_operands(storage: str, shape, seed: int, *, with_ab: bool, device="cpu"):
    """inputs of the bounded (ELU / sigmoid / tanh) cases: t = a x + b inside [-16, 8]"""
    g = torch.Generator().manual_seed(int(seed))
    dt = DTYPES[storage]
    x = (torch.rand(shape, generator=g) * 12.0 - 8.0).to(dt)
    da = torch.randn(shape, generator=g).to(dt)
    ab = None
    if with_ab:
        N, C = shape[0], shape[-1]
        ab = torch.stack([torch.rand(N, C, generator=g) + 0.5, torch.rand(N, C, generator=g) * 4.0 - 2.0], 1).contiguous()
    return x.to(device), da.to(device), (ab.to(device) if ab is not None else None)


def smooth_bound(kind: str, ref: torch.Tensor, storage: str, *, t=None, ab: bool = False) -> torch.Tensor:
    """|kernel - fp64| allowed for a smooth activation: the measured intrinsic margin, the rounding of t = fma(x, a, b) in fp32
    carried through a function of slope <= 1 (u |t|), and for bf16 storage (8 significant bits) half an ulp of the stored result,
    at most 2^-8 of it"""
    b = torch.full_like(ref, INTRINSIC_MARGIN[kind])
    if ab and t is not None:
        b = b + U32 * t.abs()
    if storage == "bf16":
        b = b + 2.0 ** -8 * ref.abs() + 2.0 ** -134
    else:
        b = b + U32 * ref.abs()
    return b


# ---------------------------------------------------------------------------------------------------------------- max pooling
POOL_SHAPES = [(2, 7, 11, 13, 5), (2, 7, 11, 13, 24)]
POOL_FACTORS = [(1, 2, 2), (2, 2, 2), (3, 2, 1), (2, 5, 3)]


def pool_input(shape, seed: int, dtype) -> torch.Tensor:
    """integers in [-3, 3]: seven values over windows of up to 30 voxels, so nearly every window has tied maxima"""
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(-3, 4, shape, generator=g).to(dtype)


def pool_grad(shape, factor, seed: int, dtype) -> torch.Tensor:
    """nonzero integer output gradients (1 .. 4, signed), so that a misrouted or dropped one is seen"""
    g = torch.Generator().manual_seed(int(seed) + 1)
    oshape = (shape[0],) + tuple(shape[1 + i] // factor[i] for i in range(3)) + (shape[4],)
    v = torch.randint(1, 5, oshape, generator=g) * (torch.randint(0, 2, oshape, generator=g) * 2 - 1)
    return v.to(dtype)


def ref_pool(x_cl: torch.Tensor, dy_cl, factor):
    """torch's max_pool3d and its autograd on the channels-last tensor (fp64: the values are small integers) -> (y, dx) like x"""
    x = x_cl.double().permute(0, 4, 1, 2, 3).contiguous().requires_grad_(dy_cl is not None)
    y = F.max_pool3d(x, factor)
    dx = None
    if dy_cl is not None:
        y.backward(dy_cl.double().permute(0, 4, 1, 2, 3).contiguous())
        dx = x.grad.permute(0, 2, 3, 4, 1).contiguous().to(x_cl.dtype)
    return y.detach().permute(0, 2, 3, 4, 1).contiguous().to(x_cl.dtype), dx


def restate_pool(x, dy, factor, *, defect=None, init=-math.inf):
    """maxpool3d_kernel / maxpool3d_bwd_kernel on (N, D, H, W, C).  defects: tie_last (>= instead of >), rim (dx not cleared: the
    floor-dropped rim keeps its fill value).  init: the forward's starting value"""
    N, D, H, W, C = x.shape
    fz, fy, fx = factor
    Do, Ho, Wo = D // fz, H // fy, W // fx
    xf = x.float()
    xc = xf[:, :Do * fz, :Ho * fy, :Wo * fx].reshape(N, Do, fz, Ho, fy, Wo, fx, C).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(N, Do, Ho, Wo, C, -1)
    y = torch.maximum(xc.max(-1).values, torch.tensor(float(init)))
    if dy is None:
        return y.to(x.dtype), None
    K = xc.shape[-1]
    ismax = xc == xc.max(-1, keepdim=True).values
    order = torch.arange(K)
    key = torch.where(ismax, order if defect == "tie_last" else K - 1 - order, torch.tensor(-1))
    arg = key.argmax(-1, keepdim=True)
    onehot = torch.zeros_like(xc).scatter_(-1, arg, 1.0) * dy.float().unsqueeze(-1)
    dxc = onehot.reshape(N, Do, Ho, Wo, C, fz, fy, fx).permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(N, Do * fz, Ho * fy, Wo * fx, C)
    dx = torch.full(x.shape, 7.0 if defect == "rim" else 0.0)
    dx[:, :Do * fz, :Ho * fy, :Wo * fx] = dxc
    return y.to(x.dtype), dx.to(x.dtype)


def rim_mask(shape, factor) -> torch.Tensor:
    """True on the voxels that floor pooling drops"""
    m = torch.ones(shape[1:4], dtype=torch.bool)
    m[:shape[1] // factor[0] * factor[0], :shape[2] // factor[1] * factor[1], :shape[3] // factor[2] * factor[2]] = False
    return m


# ---------------------------------------------------------------------------------------------------------------- the chain
CHAIN_SPATIAL = (9, 16, 20)
CHAIN_CASES = [("group", 18, 3), ("group", 36, 4), ("instance", 18, 0), ("batch", 18, 0)]     # (kind, real channels, groups)


def pad_channels(c: int, dtype) -> int:
    q = epv(dtype)
    return c if (c <= 4 or c % q == 0) else (c + q - 1) // q * q


def chain_operands(kind: str, c_real: int, storage: str, seed: int):
    """x, da (2, 9, 16, 20, C_pad) in the storage type with an all-zero channel tail; gamma / beta (c_real) or None (instance)"""
    dt = DTYPES[storage]
    C = pad_channels(c_real, dt)
    g = torch.Generator().manual_seed(int(seed))
    shape = (2,) + CHAIN_SPATIAL + (C,)
    x = torch.randn(shape, generator=g) * 1.5 + 0.25
    da = torch.randn(shape, generator=g)
    x[..., c_real:] = 0
    da[..., c_real:] = 0
    gamma = beta = None
    if kind != "instance":
        gamma, beta = general_gamma_beta(c_real, seed + 1)
    return x.to(dt), da.to(dt), gamma, beta


def chain_ref(x, da, gamma, beta, kind: str, groups: int, c_real: int, eps: float = 1e-5, dtype=torch.float64, storage=None):
    """norm -> ELU by torch autograd in `dtype` on the real channels of the stored x / da -> dict(out, dx, dgamma, dbeta, rstd_gamma).
    dtype = float32 with `storage` given is the fp32 restatement: the output and the gradient rounded to the storage type."""
    xr = x[..., :c_real].to(dtype).permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
    g = gamma.to(dtype).clone().requires_grad_(True) if gamma is not None else None
    b = beta.to(dtype).clone().requires_grad_(True) if beta is not None else None
    if kind == "group":
        t = F.group_norm(xr, groups, g, b, eps)
    elif kind == "instance":
        t = F.instance_norm(xr, eps=eps)
    else:
        t = F.batch_norm(xr, None, None, g, b, True, 0.0, eps)
    out = F.elu(t)
    d = da[..., :c_real].to(dtype).permute(0, 4, 1, 2, 3).contiguous()
    if storage is None:
        out.backward(d)
    else:       # the kernels' roundings: act'(t) of the stored-precision t, dt rounded to the storage type before the norm backward
        tr = t.detach().to(storage).to(dtype)
        t.backward((d * torch.where(tr > 0, torch.ones_like(tr), torch.exp(tr))).to(storage).to(dtype))
    cl = lambda v: v.detach().permute(0, 2, 3, 4, 1).contiguous()                # noqa: E731
    o, dx = cl(out), cl(xr.grad)
    if storage is not None:
        o, dx = o.to(storage).to(dtype), dx.to(storage).to(dtype)
    return dict(out=o, dx=dx, dgamma=None if g is None else g.grad.detach(), dbeta=None if b is None else b.grad.detach())


def rel_l2(got: torch.Tensor, want: torch.Tensor) -> float:
    return float((got.double() - want.double()).norm() / want.double().norm().clamp_min(1e-300))

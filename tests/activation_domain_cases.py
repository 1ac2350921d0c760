"""GELU, sigmoid and tanh over the whole bf16 grid: inputs, numpy interval models of the device functions and the table of entry
points that evaluate them (tests/test_host_activation_domain_cases.py proves the models and the table's premises on the host,
tests/test_gpu_activation_domain.py sweeps the kernels).  Plain numpy / torch-CPU, nothing here touches a GPU.

Inputs.  bf16_all(): all 65 536 bf16 bit patterns, pattern i at flat index i, as fp32 values in a (2048, 32) matrix.  f32_grid(): every
finite bf16 value, its two fp32 neighbours, the fp32 midpoint to the next bf16 value, 2^18 equally spaced points of [-10, 10] and the
points +-3.75, +-8 and x^2 = 64 -+ 1 ulp; zero-padded to 2^19 elements, (16384, 32).

Models.  One restatement per device function, operation by operation as csrc/pytc_common.h and csrc/pw_common.h have it: fp32
arithmetic (numpy float32 is IEEE single), fmaf as the exact fp64 product-and-sum rounded once, and every transcendental as the
correctly rounded fp64 value moved by k units, |k| <= B, B that intrinsic's budget.  The budgets are NOT taken from the kernels under
test: tools/probes/intrinsic_ulp_probe.hip evaluates each intrinsic alone and profiles/activation_domain_probe.txt records its output
and the budgets derived from it (largest error, rounded up to a whole unit, plus one).  A unit is the fp32 spacing at the reference,
2^-126 below the normal range (the hardware instructions flush there).  interval() returns [lo, hi] over all nudges, widened by one
ulp of the result for a contraction the compiler may or may not take, with the store rounding applied to both ends."""
from __future__ import annotations

import functools
import itertools
from dataclasses import dataclass

import numpy as np
import torch

F = np.float32
D = np.float64

# ---- budgets: profiles/activation_domain_probe.txt ("budget" lines), measured by tools/probes/intrinsic_ulp_probe.hip
BUDGET = {"exp2": 2, "rcp": 2, "erff": 3, "tanhf": 3}
BUDGET["expf"] = BUDGET["exp2"]          # see EXPF_IS_EXP2_OF_PRODUCT below


# ------------------------------------------------------------------------------------------------------------------ inputs
def bf16_bits_to_f32(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << 16).view(F)


@functools.lru_cache(maxsize=None)
def _bf16_all() -> np.ndarray:
    v = bf16_bits_to_f32(np.arange(65536, dtype=np.uint32)).reshape(2048, 32)
    v.setflags(write=False)
    return v


def bf16_all() -> np.ndarray:
    """all 65 536 bf16 patterns as fp32 values, (2048, 32), pattern i at flat index i (read-only, shared)"""
    return _bf16_all()


def round_bf16(v: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 (round to nearest even, NaN stays NaN) -> fp32: from_f32<bf16_t> followed by to_f32"""
    v = np.asarray(v, dtype=F)
    u = v.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16).astype(np.uint32).view(F)
    return np.where(np.isnan(v), F(np.nan), r).astype(F)


def to_bf16_tensor(v: np.ndarray) -> torch.Tensor:
    """fp32 values that ARE bf16 numbers (or NaNs) -> torch.bfloat16 with the same upper 16 bits"""
    hi = (np.ascontiguousarray(v, dtype=F).view(np.uint32) >> 16).astype(np.uint16)
    return torch.from_numpy(hi.view(np.int16).copy()).view(torch.bfloat16).reshape(v.shape)


def from_bf16_tensor(t: torch.Tensor) -> np.ndarray:
    bits = t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
    return bf16_bits_to_f32(bits).reshape(tuple(t.shape))


GRID_SHAPE = (16384, 32)


@functools.lru_cache(maxsize=None)
def _f32_grid() -> np.ndarray:
    b = bf16_all().ravel()
    fin = b[np.isfinite(b)]
    up, dn = np.nextafter(fin, F(np.inf)), np.nextafter(fin, F(-np.inf))
    # the fp32 midpoint between a bf16 value and the next one away from zero: bit 15 set
    mid = (fin.view(np.uint32) | np.uint32(0x8000)).view(F)
    eight = F(8.0)
    special = np.array([3.75, -3.75, 8.0, -8.0, np.nextafter(eight, F(0)), np.nextafter(eight, F(9)),
                        -np.nextafter(eight, F(0)), -np.nextafter(eight, F(9))], dtype=F)
    g = np.concatenate([fin, up, dn, mid, np.linspace(-10.0, 10.0, 1 << 18).astype(F), special])
    g = g[np.isfinite(g)]
    assert g.size <= 1 << 19
    out = np.zeros(1 << 19, dtype=F)
    out[:g.size] = g
    out = out.reshape(GRID_SHAPE)
    out.setflags(write=False)
    return out


def f32_grid() -> np.ndarray:
    """the fp32 sweep, (16384, 32), finite values only (read-only, shared)"""
    return _f32_grid()


# ------------------------------------------------------------------------------------------------------------------ fp32 steps
def _f(v):
    return np.asarray(v, dtype=F)


def fma(a, b, c):
    """fmaf: exact product (48 bits fit fp64) plus the addend, one rounding to fp32"""
    with np.errstate(all="ignore"):
        return (_f(a).astype(D) * _f(b).astype(D) + _f(c).astype(D)).astype(F)


def unit(r):
    """the error unit of a transcendental at its correctly rounded value r: the fp32 spacing, 2^-126 below the normal range"""
    a = np.abs(_f(r))
    with np.errstate(all="ignore"):
        s = np.spacing(np.where(np.isfinite(a), a, F(1.0)).astype(F))
    return np.where(a < F(2.0 ** -126), F(2.0 ** -126), s).astype(F)


def nudged(ref64, k: int, *, nonneg: bool = False):
    """the correctly rounded fp32 value of ref64 moved by k units; 0, inf and NaN stay as they are, and so does a reference that IS an
    fp32 number (a reciprocal of a power of two, 2^integer, f(0)): the probe finds the instructions exact there ("exact cases" lines),
    and gelu_fast_with_grad's 1 - s depends on rcp(1) = 1 for every x > 5"""
    with np.errstate(all="ignore"):
        r = np.asarray(ref64, dtype=D).astype(F)
        if k == 0:
            return r
        keep = ~np.isfinite(r) | (np.asarray(ref64, dtype=D) == r.astype(D))
        m = (r.astype(D) + k * unit(r).astype(D)).astype(F)
        if nonneg:
            m = np.maximum(m, F(0))
        return np.where(keep, r, m).astype(F)


# __expf compiles to v_exp_f32(x * log2(e)): the probe compares the two bit for bit ("__expf(v) != v_exp_f32(v * log2e) at 0 arguments"),
# so the models restate it as that fp32 product and the nudged instruction.  Against exp() itself its error grows with |x| (the
# product's rounding is scaled by the argument): the probe's "expf" lines, up to tens of units at x = -100.
EXPF_IS_EXP2_OF_PRODUCT = True


def expf(arg, k: int):
    """__expf(arg), arg fp32"""
    with np.errstate(all="ignore"):
        if EXPF_IS_EXP2_OF_PRODUCT:
            return nudged(np.exp2((_f(arg) * LOG2E).astype(D)), k, nonneg=True)
        return nudged(np.exp(_f(arg).astype(D)), k, nonneg=True)


def _erf64(v):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(v, dtype=D))).numpy()


# ---- the device functions; k* are the nudges of their transcendentals, `defect` a seeded change (discrimination tests only)
SQRT1_2 = F(0.70710678118654752440)
LOG2E = F(1.44269504088896340736)
INV_SQRT_2PI = F(0.3989422804014327)
AS_C = (0.3275911, 1.061405429, -1.453152027, 1.421413741, -0.284496736, 0.254829592)
FAST_C = (1.0142630e-3, -1.0677572e-1, -2.3011213)


def _as_parts(x, kr, ke, defect):
    """az, p(t) t, e = exp(-x^2/2) of gelu_erf / gelu_erf_grad"""
    c = list(AS_C)
    if defect == "as_coef":
        c[0] = 0.3275912                                     # last printed digit (the other five are the same fp32 number either way)
    with np.errstate(all="ignore"):
        az = np.abs(x) * SQRT1_2
        t = nudged(1.0 / fma(F(c[0]), az, F(1.0)).astype(D), kr)
        p = fma(t, F(c[1]), F(c[2]))
        p = fma(t, p, F(c[3]))
        p = fma(t, p, F(c[4]))
        p = fma(t, p, F(c[5]))
        p = p * t
        e = nudged(np.exp2(((-az * az) * LOG2E).astype(D)), ke, nonneg=True)
    return p, e


def gelu_erf(x, kr=0, ke=0, defect=None):
    x = _f(x)
    with np.errstate(all="ignore"):
        p, e = _as_parts(x, kr, ke, defect)
        neg = (x <= 0) if defect == "le" else (x < 0)
        return ((F(0.5) * x) * np.where(neg, p * e, fma(-p, e, F(2.0)))).astype(F)


def gelu_erf_grad(x, kr=0, ke=0, defect=None):
    x = _f(x)
    with np.errstate(all="ignore"):
        p, e = _as_parts(x, kr, ke, defect)
        neg = (x <= 0) if defect == "le" else (x < 0)
        return fma(x * INV_SQRT_2PI, e, F(0.5) * np.where(neg, p * e, fma(-p, e, F(2.0))))


def _fast_parts(x, ke, kr, defect):
    c = list(FAST_C)
    if defect == "fast_coef":
        c[0] = 1.0142631e-3
    with np.errstate(all="ignore"):
        x2 = x * x if defect == "no_clamp" else np.fmin(x * x, F(64.0))
        p = fma(x2, F(c[0]), F(c[1]))
        p = fma(p, x2, F(c[2]))
        e = nudged(np.exp2((x * p).astype(D)), ke, nonneg=True)
        s = nudged(1.0 / (F(1.0) + e).astype(D), kr)
    return x2, p, e, s, c


def gelu_fast(x, ke=0, kr=0, defect=None):
    x = _f(x)
    with np.errstate(all="ignore"):
        _, _, _, s, _ = _fast_parts(x, ke, kr, defect)
        return (x * s).astype(F)


def gelu_fast_grad(x, ke=0, kr=0, defect=None):
    """gd of gelu_fast_with_grad (its g is gelu_fast, operation for operation)"""
    x = _f(x)
    with np.errstate(all="ignore"):
        x2, p, e, s, c = _fast_parts(x, ke, kr, defect)
        g = x * s
        q = fma(x2, F(2.0) * F(c[0]), F(c[1]))
        du = fma(x2 + x2, q, p)
        tail = e * s if defect == "e_times_s" else F(1.0) - s
        return fma(g * tail, du * F(-0.69314718055994530942), s)


def gelu_grad_libm(x, kf=0, kx=0, defect=None):
    """gelu_grad (pytc_common.h): Phi(x) + x phi(x) with libm erff and __expf"""
    x = _f(x)
    with np.errstate(all="ignore"):
        if defect == "as_erf":                               # erff swapped for the A&S form: 1 + erf from gelu_erf's pieces
            p, e = _as_parts(x, 0, 0, None)
            phi_big = F(0.5) * np.where(x < 0, p * e, fma(-p, e, F(2.0)))
        else:
            phi_big = F(0.5) * (F(1.0) + nudged(_erf64((x * SQRT1_2).astype(D)), kf))
        pdf = INV_SQRT_2PI * expf(F(-0.5) * x * x, kx)
        return (phi_big + x * pdf).astype(F)


def sigmoid(x, kx=0, defect=None):
    x = _f(x)
    with np.errstate(all="ignore"):
        return (F(1.0) / (F(1.0) + expf(-x, kx))).astype(F)


def tanh(x, kt=0, defect=None):
    x = _f(x)
    with np.errstate(all="ignore"):
        return nudged(np.tanh(x.astype(D)), kt)


# function name -> (model, budgets of its two / one transcendentals in call order)
MODELS = {
    "gelu_erf": (gelu_erf, ("rcp", "exp2")),
    "gelu_erf_grad": (gelu_erf_grad, ("rcp", "exp2")),
    "gelu_fast": (gelu_fast, ("exp2", "rcp")),
    "gelu_fast_grad": (gelu_fast_grad, ("exp2", "rcp")),
    "gelu_grad_libm": (gelu_grad_libm, ("erff", "expf")),
    "sigmoid": (sigmoid, ("expf",)),
    "tanh": (tanh, ("tanhf",)),
}


def _nudges(b: int):
    return range(-b, b + 1) if b <= 3 else (-b, -(b // 2), 0, b // 2, b)


def store(v, dtype: str):
    return round_bf16(v) if dtype == "bf16" else _f(v)


@dataclass(frozen=True)
class Interval:
    lo: np.ndarray        # fp32; NaN where every nudge gives NaN
    hi: np.ndarray
    nan_ok: np.ndarray    # some nudge gives NaN
    num_ok: np.ndarray    # some nudge gives a number


def interval(fn: str, x: np.ndarray, *, mid: str | None = None, out: str = "f32", defect=None) -> Interval:
    """[lo, hi] of device function `fn` at x over all nudges within the budgets, widened by one ulp of the result, then rounded to
    `mid` (the type an activation is rounded to before an exact GEMM carries it on; None: not rounded) and to the storage type `out`.
    defect: a seeded change to the model (discrimination tests only)."""
    model, kinds = MODELS[fn]
    x = _f(x)
    lo = np.full(x.shape, np.inf, dtype=F)
    hi = np.full(x.shape, -np.inf, dtype=F)
    nan_ok = np.zeros(x.shape, dtype=bool)
    num_ok = np.zeros(x.shape, dtype=bool)
    for ks in itertools.product(*[_nudges(BUDGET[k]) for k in kinds]):
        v = model(x, *ks, defect=defect)
        n = np.isnan(v)
        nan_ok |= n
        num_ok |= ~n
        lo = np.where(n, lo, np.minimum(lo, v))
        hi = np.where(n, hi, np.maximum(hi, v))
    with np.errstate(all="ignore"):
        lo = np.where(np.isfinite(lo), lo - np.spacing(np.abs(lo)), lo).astype(F)
        hi = np.where(np.isfinite(hi), hi + np.spacing(np.abs(hi)), hi).astype(F)
    for t in (mid, out):
        if t == "bf16":
            lo, hi = round_bf16(lo), round_bf16(hi)
    lo = np.where(num_ok, lo, F(np.nan))
    hi = np.where(num_ok, hi, F(np.nan))
    return Interval(lo, hi, nan_ok, num_ok)


def inside(iv: Interval, got: np.ndarray) -> np.ndarray:
    """elementwise: got lies in the interval (NaN only where a NaN is allowed; -0 and +0 compare equal here, see zero_sign_ok)"""
    got = _f(got)
    n = np.isnan(got)
    with np.errstate(all="ignore"):
        return np.where(n, iv.nan_ok, iv.num_ok & (got >= iv.lo) & (got <= iv.hi))


def against_central(fn: str, x: np.ndarray, got: np.ndarray, *, mid, out: str):
    """(inputs at which the stored result differs from the UN-NUDGED model's bits, largest absolute difference): information for the
    probe file -- how much of the budget the hardware actually uses"""
    c = _f(MODELS[fn][0](_f(x)))
    if mid == "bf16":
        c = round_bf16(c)
    c = store(c, out)
    g = _f(got)
    with np.errstate(all="ignore"):
        ok = np.isfinite(c) & np.isfinite(g)
        d = np.abs(g[ok].astype(D) - c[ok].astype(D))
    return int((d != 0).sum()), float(d.max()) if d.size else 0.0


def position(iv: Interval, got: np.ndarray) -> float:
    """the worst observed position inside [lo, hi]: max |got - centre| / half-width over the finite intervals wider than a point"""
    with np.errstate(all="ignore"):
        lo, hi, g = iv.lo.astype(D), iv.hi.astype(D), _f(got).astype(D)
        ok = np.isfinite(lo) & np.isfinite(hi) & (hi > lo) & np.isfinite(g)
        if not ok.any():
            return 0.0
        return float(np.max(np.abs(g[ok] - 0.5 * (lo[ok] + hi[ok])) / (0.5 * (hi[ok] - lo[ok]))))


def describe_failures(entry: str, x: np.ndarray, got: np.ndarray, iv: Interval, bad: np.ndarray, limit: int = 5) -> str:
    idx = np.flatnonzero(bad.ravel())[:limit]
    xs, gs, lo, hi = _f(x).ravel(), _f(got).ravel(), iv.lo.ravel(), iv.hi.ravel()
    rows = [f"x={xs[i]!r} (bits 0x{int(xs[i:i + 1].view(np.uint32)[0]):08x}) got={gs[i]!r} lo={lo[i]!r} hi={hi[i]!r}" for i in idx]
    return f"{entry}: {int(bad.sum())} outputs outside their interval, e.g. " + "; ".join(rows)


# ------------------------------------------------------------------------------------------------------------------ fp64 references
def gelu64(x):
    x = np.asarray(x, dtype=D)
    with np.errstate(all="ignore"):
        return 0.5 * x * (1.0 + _erf64(x * np.sqrt(0.5)))


def gelu_grad64(x):
    x = np.asarray(x, dtype=D)
    with np.errstate(all="ignore"):
        return 0.5 * (1.0 + _erf64(x * np.sqrt(0.5))) + x * np.exp(-0.5 * x * x) / np.sqrt(2.0 * np.pi)


def _as_one_plus_erf64(z):
    """the A&S 7.1.26 form of 1 + erf(z) in fp64 (the formula without fp32 roundings)"""
    a = np.abs(z)
    t = 1.0 / (1.0 + AS_C[0] * a)
    p = ((((AS_C[1] * t + AS_C[2]) * t + AS_C[3]) * t + AS_C[4]) * t + AS_C[5]) * t
    pe = p * np.exp(-a * a)
    return np.where(z < 0, pe, 2.0 - pe)


def gelu_erf64(x):
    x = np.asarray(x, dtype=D)
    return 0.5 * x * _as_one_plus_erf64(x * np.sqrt(0.5))


def gelu_erf_grad64(x):
    x = np.asarray(x, dtype=D)
    return 0.5 * _as_one_plus_erf64(x * np.sqrt(0.5)) + x * np.exp(-0.5 * x * x) / np.sqrt(2.0 * np.pi)


def gelu_erf_true_grad64(x):
    """the analytic derivative OF gelu_erf64 (A&S erf differentiated as a formula), not of the exact GELU"""
    x = np.asarray(x, dtype=D)
    z = x * np.sqrt(0.5)
    a = np.abs(z)
    t = 1.0 / (1.0 + AS_C[0] * a)
    p = ((((AS_C[1] * t + AS_C[2]) * t + AS_C[3]) * t + AS_C[4]) * t + AS_C[5]) * t
    dp_dt = (((5 * AS_C[1] * t + 4 * AS_C[2]) * t + 3 * AS_C[3]) * t + 2 * AS_C[4]) * t + AS_C[5]
    e = np.exp(-a * a)
    dpe_da = (dp_dt * (-AS_C[0] * t * t) - 2.0 * a * p) * e          # d/da [p(t(a)) exp(-a^2)]
    # 1 + erf(z) = pe (z < 0) | 2 - pe (z >= 0) and a = |z|: d/dz is -dpe_da on both sides
    return 0.5 * _as_one_plus_erf64(z) + 0.5 * x * (-dpe_da) * np.sqrt(0.5)


def _fast_u64(x):
    x2 = np.minimum(x * x, 64.0)
    c0, c1, c2 = (float(F(v)) for v in FAST_C)
    return x2, x * ((c0 * x2 + c1) * x2 + c2), c0, c1, c2


def gelu_fast64(x):
    x = np.asarray(x, dtype=D)
    with np.errstate(all="ignore"):
        _, u, *_ = _fast_u64(x)
        return x / (1.0 + np.exp2(u))


def gelu_fast_grad64(x):
    """the analytic derivative of gelu_fast64 inside the clamp, the formula gelu_fast_with_grad states outside it"""
    x = np.asarray(x, dtype=D)
    with np.errstate(all="ignore"):
        x2, u, c0, c1, c2 = _fast_u64(x)
        s = 1.0 / (1.0 + np.exp2(u))
        du = ((c0 * x2 + c1) * x2 + c2) + 2.0 * x2 * (2.0 * c0 * x2 + c1)
        return s + x * s * (1.0 - s) * (-np.log(2.0)) * du


FUNCTION64 = {"gelu_erf": gelu_erf64, "gelu_fast": gelu_fast64, "gelu_erf_grad": gelu_erf_grad64, "gelu_fast_grad": gelu_fast_grad64,
              "gelu_grad_libm": gelu_grad64}
DERIVATIVE64 = {"gelu_erf": gelu_erf_true_grad64, "gelu_fast": gelu_fast_grad64}


# ------------------------------------------------------------------------------------------------------------------ entry points
@dataclass(frozen=True)
class Entry:
    id: str
    call: str             # the hip_ops call
    route: str            # the kernel, and what picks it
    din: str              # dtype of the swept operand
    dout: str             # dtype of the checked result
    fn: str               # the device function evaluated (key of MODELS)
    mid: str | None       # type the activation is rounded to before an exact step carries it to the store (None: only the store rounds)
    recipe: str           # key of RECIPES: the operands that isolate the activation
    width: int            # channels of the swept operand as the launch sees it (the sweep is reshaped to (-1, width))
    sweep: tuple = ("bf16_all",)

    @property
    def spec(self):
        return RECIPES[self.recipe]

    @property
    def group(self):
        """entries with the same key must return identical VALUES, bit for bit as fp32, for every finite input (a zero result compared
        without its sign where one of the two passes an accumulator, Recipe.zero_sign_lost).  The key is the function, the input type and
        the type the activation is rounded to: a bf16-rounded activation carried exactly into an fp32 weight gradient is the same number
        as the one a bf16 store holds, so `dout` is not part of it"""
        return (self.fn, self.din, self.mid or self.dout)


@dataclass(frozen=True)
class Recipe:
    text: str             # how the activation is isolated
    shares_sum: bool      # swept values share a GEMM sum (0 * inf = NaN would pollute it): non-finite inputs are swept as 0 there
    zero_sign_lost: bool  # the value passes an accumulator that starts at +0: 0 + -0 = +0, the sign of a zero result is not kept


RECIPES = {
    "elementwise": Recipe("none needed", False, False),
    "grn": Recipe("A = 1, B = 0, dh2 = 1: dh = fmaf(1, 1, h * 0) = 1 for every finite h; times g'(hp)", False, False),
    "ones_times_grad": Recipe("GEMM operand rows of ones against a (stacked) identity: every output is the single product 1 * 1, "
                              "the epilogue multiplies it by g'(res)", False, False),
    "identity_after": Recipe("W = zero-padded identity, bias 0: the accumulator is 0 + 1 * x, the activation follows", True, True),
    "identity_before": Recipe("W = zero-padded identity, bias 0: the activation is the GEMM operand, every output 0 + 1 * g(x)", True, True),
    "stem": Recipe("C_in = 1, w = 1 on 8 output channels, bias 0: fmaf(1, x, 0) per channel, all 8 must agree", False, True),
    "head": Recipe("C_out = 1, C_in = 8, w = e_0, the other seven inputs 0: fmaf chain 1 * x + 0 * 0 ...", False, True),
    "onehot_wgrad": Recipe("R rows, dy = I (R x R): dW[o][k] = 1 * g(x[o][k]) + (R - 1) zeros", True, True),
    "mixer": Recipe("affine (1, 0), W2 = [I; 0] (64 x 32), b2 = 0: the hidden pre-activation is x beside 32 zero channels; W3 = [I | 0] (32 x 64), "
                    "b3 = 0: y = g(hp) of the first 32 hidden channels, every GEMM output a single product", True, True),
    "rebuilt": Recipe("mixer_bwd_rc rebuilds hp = W2 (1 t + 0) + 0 with W2 = I stacked (C_hid x 32): hp = t in every 32-channel group, each a single "
                      "product; 32 rows, dy = I, W3 = ones: (W3^T dy) = 1 and dW3[o][k] = g(hp[o][k]); every group must agree", True, True),
    "onehot_row": Recipe("pw_mlp_bwd: identity affine, dy = e_0 in every row, W3 = first row of ones: (W3^T dy)[k] is the single product 1 * 1, "
                         "times g'(hidden_pre); W2 = 0 and dx is not read", False, False),
    "onehot_dgrad": Recipe("32 rows, dy = I (32 x 32), W = ones: (W^T dy)[r][k] = the single product 1 * 1, times g'(hp)", False, False),
}


def _rows():
    E = Entry
    out = []
    for dt in ("f32", "bf16"):
        sw = ("bf16_all", "f32_grid") if dt == "f32" else ("bf16_all",)
        out += [
            E(f"gelu.fwd.{dt}", "ops.gelu(x)", "gelu_kernel", dt, dt, "gelu_erf", None, "elementwise", 32, sw),
            E(f"gelu.bwd.{dt}", "ops.gelu(x, dy=1)", "gelu_kernel", dt, dt, "gelu_grad_libm", None, "elementwise", 32, sw),
            E(f"grn_bwd_apply.{dt}", "ops.grn_bwd_apply", "grn_bwd_apply_kernel", dt, dt, "gelu_grad_libm", None, "grn", 32, sw),
            E(f"pw_conv.res_gelu_bwd.generic.{dt}", "ops.pw_conv(res_mode=RES_GELU_BWD)", f"pw_conv_kernel, {dt} weights", dt, dt,
              "gelu_erf_grad", None, "ones_times_grad", 32, sw),
            E(f"linear_bwd.plain.{dt}", "ops.linear_bwd(x_gelu=True) dx", "linear_gemm_kernel (32 -> 32)", dt, dt, "gelu_erf_grad", None,
              "ones_times_grad", 32, sw),
            E(f"pw_conv.pre_act.generic.{dt}", "ops.pw_conv(pre_act=GELU)", f"pw_conv_kernel, {dt} weights", dt, dt, "gelu_erf",
              "bf16" if dt == "bf16" else None, "identity_before", 32, sw),
            E(f"linear_fwd.plain.{dt}", "ops.linear_fwd(x_gelu=True)", "linear_gemm_kernel (32 -> 32)", dt, dt, "gelu_erf", None,
              "identity_before", 32, sw),
        ]
        for act in ("gelu", "sigmoid", "tanh"):
            fn = "gelu_erf" if act == "gelu" else act
            out.append(E(f"pw_conv.act.{act}.generic.{dt}", f"ops.pw_conv(act={act.upper()})", f"pw_conv_kernel, {dt} weights", dt, dt, fn, None,
                         "identity_after", 32, sw))
    for act in ("gelu", "sigmoid", "tanh"):
        fn = "gelu_erf" if act == "gelu" else act
        out += [
            E(f"pw_conv.act.{act}.stem", f"ops.pw_conv(act={act.upper()})", "pw_stem_kernel (C_in = 1)", "bf16", "bf16", fn, None, "stem", 1),
            E(f"pw_conv.act.{act}.head", f"ops.pw_conv(act={act.upper()})", "pw_head_kernel (C_out = 1)", "bf16", "bf16", fn, None, "head", 1),
        ]
    B = "bf16"
    out += [
        E("pw_conv.pre_act.paired", "ops.pw_conv(pre_act=GELU, w_paired=1)", "pw_fast_kernel (32 -> 32)", B, B, "gelu_fast", B, "identity_before", 32),
        E("pw_conv.pre_act.rowmajor", "ops.pw_conv(pre_act=GELU, w_paired=2)", "pw_gemm_lds_kernel (64 -> 128)", B, B, "gelu_fast", B,
          "identity_before", 64),
        E("linear_fwd.mfma", "ops.linear_fwd(x_gelu=True)", "pw_gemm_lds_kernel (64 -> 128) via linear_mfma_applies", B, B, "gelu_fast", B,
          "identity_before", 64),
        E("pw_conv.res_gelu_bwd.paired", "ops.pw_conv(res_mode=RES_GELU_BWD, w_paired=1)", "pw_fast_kernel (32 -> 32)", B, B, "gelu_erf_grad",
          None, "ones_times_grad", 32),
        E("pw_conv.res_gelu_bwd.rowmajor", "ops.pw_conv(res_mode=RES_GELU_BWD, w_paired=2)", "pw_gemm_lds_kernel (64 -> 128)", B, B,
          "gelu_erf_grad", None, "ones_times_grad", 128),
        E("linear_bwd.mfma", "ops.linear_bwd(x_gelu=True) dx", "pw_gemm_lds_kernel (64 -> 128) via linear_mfma_applies", B, B, "gelu_erf_grad",
          None, "ones_times_grad", 128),
        E("pw_wgrad.valu.bf16", "ops.pw_wgrad(x_act=GELU), wgrad_valu = 1", "pw_wgrad_kernel<bf16>", B, "f32", "gelu_erf", B, "onehot_wgrad", 1024),
        E("pw_wgrad.valu.f32", "ops.pw_wgrad(x_act=GELU)", "pw_wgrad_kernel<float>", "f32", "f32", "gelu_erf", None, "onehot_wgrad", 1024,
          ("bf16_all", "f32_grid")),
        E("pw_wgrad.mfma", "ops.pw_wgrad(x_act=GELU), wgrad_valu = 0", "pw_wgrad_mfma_kernel<4, 4>", B, "f32", "gelu_fast", B, "onehot_wgrad", 1024),
        E("linear_bwd.plain.dW", "ops.linear_bwd(x_gelu=True) dW", "linear_gemm_kernel (dy^T gelu(x))", "f32", "f32", "gelu_erf", None,
          "onehot_wgrad", 1024, ("bf16_all", "f32_grid")),
        E("linear_bwd.plain.dW.bf16", "ops.linear_bwd(x_gelu=True) dW", "linear_gemm_kernel (dy^T gelu(x)), bf16 x: gelu_erf is NOT rounded", B, "f32",
          "gelu_erf", None, "onehot_wgrad", 1024),
        E("pw_mlp_bwd.d_hidden", "ops.pw_mlp_bwd d_hidden", "pw_mlp_kernel, backward form (32 -> 64 -> 32)", B, B, "gelu_erf_grad", None, "onehot_row", 64),
    ]
    out += [
        E("pw_mlp.train.stored", "ops.pw_mlp(hidden_pre=...)", "pw_mlp_kernel, training form (32 -> 64 -> 32)", B, B, "gelu_fast", B, "mixer", 32),
        E("pw_mlp.train.nostore", "ops.pw_mlp(train_nostore=True)", "pw_mlp_kernel, training form without the store", B, B, "gelu_fast", B,
          "mixer", 32),
    ]
    for cin, kernel, grad in ((32, "pw_wgrad_mfma_kernel<2, 2, true>", "gelu_erf_grad"), (64, "pw_wgrad_mfma_kernel<2, 4, true>", "gelu_erf_grad"),
                              (128, "pw_wgrad_dgrad_wide_kernel<8>", "gelu_fast_grad")):
        out += [
            E(f"pw_wgrad_dgrad.{cin}.dW", "ops.pw_wgrad_dgrad dW", kernel, B, "f32", "gelu_fast", B, "onehot_wgrad", cin),
            E(f"pw_wgrad_dgrad.{cin}.dhp", "ops.pw_wgrad_dgrad dhp", kernel, B, B, grad, None, "onehot_dgrad", cin),
        ]
    for chid in (32, 64):
        out += [
            E(f"mixer_bwd_rc.{chid}.dW3", "ops.mixer_bwd_rc dW3", f"mixer_bwd_rc_kernel<{chid // 16}, false>", B, "f32", "gelu_fast", B, "rebuilt", 32),
            E(f"mixer_bwd_rc.{chid}.dhp", "ops.mixer_bwd_rc dhp", f"mixer_bwd_rc_kernel<{chid // 16}, false>", B, B, "gelu_fast_grad", None, "rebuilt", 32),
        ]
    return tuple(out)


ENTRIES = _rows()
BY_ID = {e.id: e for e in ENTRIES}

# entry points that evaluate one of these functions and are NOT swept here, each with its reason (DESIGN.md 4.3c repeats them)
NOT_COVERED = {
    "ops.mixer_bwd_rc at C_hid = 96 and its GroupNorm form": "the same kernel template as the swept C_hid = 32 / 64 launches (HT = 6; GN adds sums, not "
                                                             "another activation)",
    "ops.pw_mlp_up": "pw_mlp_up_kernel evaluates gelu_fast rounded to bf16 behind a transposed depthwise conv formed in the kernel; operands that "
                     "make that stencil hand one value through were not worked out here, the launch is not written",
    "gelu_h2 / gelu_h8_from_f32": "tests/mixer_exact_cases.py has the bit model (gelu_h2_model) and sweeps it",
}


def sweep_values(e: Entry, sweep: str) -> np.ndarray:
    """the fp32 values entry e is swept over, (-1, e.width): bf16_all() or f32_grid(), non-finite values swept as 0 where they would
    share a sum with finite ones (their classes are checked on the entries of the same function that keep them)"""
    x = (bf16_all() if sweep == "bf16_all" else f32_grid()).reshape(-1, e.width)
    if e.spec.shares_sum:
        x = np.where(np.isfinite(x), x, F(0)).astype(F)
    return x


def expected(e: Entry, x: np.ndarray) -> Interval:
    return interval(e.fn, x, mid=e.mid, out=e.dout)


def zero_padded_identity(rows: int, cols: int) -> np.ndarray:
    """(rows, cols) fp64: I stacked / tiled so that every row and every column of the smaller extent has exactly one 1"""
    w = np.zeros((rows, cols), dtype=D)
    if rows >= cols:
        w[np.arange(rows), np.arange(rows) % cols] = 1.0
    else:
        w[np.arange(cols) % rows, np.arange(cols)] = 1.0
    return w


def top_identity(rows: int, cols: int) -> np.ndarray:
    """[I; 0] (rows >= cols): output channel o < cols reads input channel o, the other outputs read nothing"""
    w = np.zeros((rows, cols), dtype=D)
    w[np.arange(cols), np.arange(cols)] = 1.0
    return w


def one_term_gemm(a: np.ndarray, w: np.ndarray) -> np.ndarray:
    """a (R, K) @ w^T (C_out, K) in fp64, asserting that every output is a sum with AT MOST ONE non-zero term: then every partial sum in
    any order, on any unit (FMA chain, MFMA), is that term or 0, an fp32 number -- the GEMM around the activation is exact"""
    a, w = np.asarray(a, dtype=D), np.asarray(w, dtype=D)
    terms = (a != 0).astype(np.int64) @ (w != 0).astype(np.int64).T
    assert terms.max() <= 1, "an output has more than one non-zero term"
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(a), a, 0.0) @ w.T


# ------------------------------------------------------------------------------------------------------------------ pairing table
@dataclass(frozen=True)
class Pairing:
    schedule: str         # the training schedule (training/autograd.py, training/transformer_autograd.py)
    forward: str          # function the forward evaluated
    backward: str         # derivative the backward applies
    same: bool            # the backward's formula is the derivative of the forward's own function
    bound: float          # max |f'_applied - d/dx f_forward| over the sweeps, fp64 formulas (asserted to three figures by the host test)


# gelu_erf_grad and gelu_grad are Phi + x phi, the derivative of the EXACT GELU, evaluated with the A&S erf / libm erff; as derivatives of
# gelu_erf itself (the A&S formula differentiated) they are off by the A&S fit's own slope error, 5.31e-7 / 5.34e-7: "same" up to that.
A_S_SLOPE = 5.31e-7
MIXED_PAIR_CLAIM = 1.1e-4     # pytc_common.h: |gelu_fast' - gelu'| over the whole axis
PAIRINGS = (
    Pairing("fp32 two-GEMM (pre_act GELU on pw_conv_kernel + RES_GELU_BWD)", "gelu_erf", "gelu_erf_grad", True, A_S_SLOPE),
    Pairing("bf16 two-GEMM (paired / row-major pre_act prologue + RES_GELU_BWD)", "gelu_fast", "gelu_erf_grad", False, MIXED_PAIR_CLAIM),
    Pairing("fused pw_mlp training forward + RES_GELU_BWD", "gelu_fast", "gelu_erf_grad", False, MIXED_PAIR_CLAIM),
    Pairing("mixer_bwd_rc", "gelu_fast", "gelu_fast_grad", True, 1e-9),
    Pairing("pw_wgrad_dgrad, C_in = 128 (pw_wgrad_dgrad_wide_kernel)", "gelu_fast", "gelu_fast_grad", True, 1e-9),
    Pairing("pw_wgrad_dgrad, C_in = 32 / 64 (pw_wgrad_mfma_kernel<.., true>)", "gelu_fast", "gelu_erf_grad", False, MIXED_PAIR_CLAIM),
    Pairing("GRN variant (ops.gelu + grn_bwd_apply)", "gelu_erf", "gelu_grad_libm", True, 5.34e-7),
    Pairing("LinearFn, plain route", "gelu_erf", "gelu_erf_grad", True, A_S_SLOPE),
    Pairing("LinearFn, MFMA route (linear_mfma_applies)", "gelu_fast", "gelu_erf_grad", False, MIXED_PAIR_CLAIM),
)

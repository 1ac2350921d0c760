"""Exact cases for the per-row LayerNorm forward and dx in its three forms: layernorm_wide_* (csrc/transformer_kernels.hip, UNETR),
layernorm_any_* (csrc/swin_kernels.hip, SwinUNETR) and layernorm_rows_* (csrc/norm_pool_kernels.hip, csrc/norm_variant_kernels.hip,
MedNeXt norm_type='layer').

Rows with an exact answer.  A row is x_c = mu + a sigma_c with sigma a balanced +-1 pattern (C / 2 of each, rolled and signed per row), a a power
of two, mu a small integer, eps = 0.  Then in fp32, in ANY summation order: sum x = C mu (integers below 2^24), mean = mu, every centred
square is a^2, their sum is C a^2, the variance is a^2, and 1 / sqrtf(a^2) = 1 / a; xhat = +-1 and y = +-gamma + beta with integer
gamma, beta.  The gradient is built as g = dy gamma = 2 (m1 + sigma m2 + h) with integers m1, m2 and h summing to zero over the +1 and
over the -1 channels separately, so sum g = 2 C m1 and sum g sigma = 2 C m2 are whole multiples of C, and
dx = (g - mean(g) - sigma mean(g sigma)) / a = 2 h / a is an exact dyadic; dgamma = sum_r dy sigma and dbeta = sum_r dy are integer sums.
`exact_rows` asserts all of this per case in numpy fp32, and |values| <= 256 for bf16.  C = 1 has no balanced pattern: there x - mean = 0,
so with eps = 1e-5 y = beta and dx = 0 exactly.

layernorm_rows_* computes 1.0f / sqrtf: equality in both types.  layernorm_wide_* and layernorm_any_* call rsqrtf.  If the device's
rsqrtf returns 2^-k at 4^k (the GPU test probes it: xhat of a +-a row must be +-1) everything is compared with equality; bf16 outputs
are integers or quarters, far from a rounding midpoint, and are compared with equality either way.  Otherwise fp32 outputs are held
to `rsqrt_bound`, derived from the statement that the hardware reciprocal square root is good to 1 ulp (2 u, u = 2^-24:
norm_act_exact_cases.py) plus the counted fp32 operations:
    rstd = (1 + d) / a, |d| <= 2 u;  xhat = fl((x - mu) rstd) = +-(1 + d1), |d1| <= 3 u;
    y = fl(fl(xhat gamma) + beta):  |y - ref| <= (4 |gamma| + |ref|) u                                          =: bound_y
    m1 exact;  s2 = sum g xhat: each product carries d1 and a rounding (4 u |g|), the C / 64-term lane sums and the 6-step wave sum
    add (C / 64 + 6) u sum|g|, the division u:  |m2 - ref| <= (C / 64 + 11) u sum|g| / C                            =: e2
    dx = fl(rstd fl(fl(g - m1) - fl(xhat m2))):  |dx - ref| <= (e2 + 3 u |m2| + 6 u (|g| + |m1| + |m2|)) / a      =: bound_dx
(first order in u; doubled for the second-order terms).  The host test asserts that the bound stays 100 x below the smallest change
any defect of the list makes.

General rows.  Integers in -3 .. 4, eps = 1e-5, dy ternary, integer gamma / beta: y and dx are checked against fp64 within the
per-element bound of `general_bounds` (derived there, the same way) plus half an ulp of the storage type.

Plain module (no tests)."""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass

import numpy as np
import torch

import exact_reduction_cases as R

U = R.U32
TORCH_DT = {"bf16": torch.bfloat16, "f32": torch.float32}

# ---- launch rules, restated (tests/test_host_layernorm_exact_cases.py reads them out of the sources)
WIDE_MAX_CHUNKS, WIDE_FWD_ROWS, WIDE_BWD_ROWS = 16, 4, 32        # C = 64 nv, nv <= 16; rows per block forward / backward
ANY_ROWS, ANY_SLOT_ROWS, ANY_MIN_C, ANY_MAX_C = 4, 256, 16, 6144  # rows per block; rows per parameter slot; C % 16 == 0
ROWS_FWD_MAX_BLOCKS, ROWS_BWD_MAX_BLOCKS = 65536, 1024


def ln_vec(C: int) -> int:
    """widest VEC <= 8 with C = VEC 2^k, 2^k <= 64; 0: refused"""
    for v in (8, 4, 2, 1):
        k = C // v
        if C % v == 0 and k >= 1 and k & (k - 1) == 0 and k <= 64:
            return v
    return 0


def rows_rpb(C: int) -> int:
    return 256 // (C // ln_vec(C))


assert R.layernorm_rows_rpb(512) == rows_rpb(512) == 4


@dataclass(frozen=True)
class LnCase:
    form: str                 # wide | any | rows
    dt: str
    C: int
    rows: int
    affine: bool = True
    kind: str = "pair"        # pair: exact rows and general rows; bwd_cap / fwd_cap: the grid caps of the rows form

    @property
    def id(self):
        return f"{self.form}-{self.dt}-c{self.C}-r{self.rows}" + ("" if self.affine else "-plain") + ("" if self.kind == "pair" else f"-{self.kind}")

    @property
    def chunk(self):
        """channels one lane-step of a row's statistic covers: a defect may lose them"""
        return 64 if self.form != "rows" else ln_vec(self.C)

    @property
    def padded(self):
        return {"wide": 64 * WIDE_MAX_CHUNKS, "any": -(-self.C // 64) * 64, "rows": self.C}[self.form]

    def block_rows(self, bwd: bool):
        if self.form == "wide":
            return WIDE_BWD_ROWS if bwd else WIDE_FWD_ROWS
        return ANY_ROWS if self.form == "any" else rows_rpb(self.C)

    @property
    def n_seq(self):
        """sequential additions one lane makes before the shuffle tree"""
        return max(1, self.C // 64) if self.form != "rows" else ln_vec(self.C)


WIDE_C, WIDE_ROWS = (64, 192, 768, 1024), (1, 3, 4, 5, 31, 32, 33, 65)
ANY_C, ANY_ROWS_SET = (16, 48, 80, 96, 1536, 6144), (1, 3, 4, 5, 257)
ROWS_C, ROWS_REFUSED = (1, 2, 4, 8, 32, 128, 512), (12, 48, 96, 1024)


def cases():
    out = []
    for dt in ("bf16", "f32"):
        out += [LnCase("wide", dt, C, r) for C in WIDE_C for r in WIDE_ROWS]
        out += [LnCase("any", dt, C, r, aff) for C in ANY_C for r in ANY_ROWS_SET for aff in (True, False)]
        for C in ROWS_C:
            rpb = rows_rpb(C)
            out += [LnCase("rows", dt, C, r) for r in sorted({1, rpb - 1, rpb, rpb + 1})]
    out.append(LnCase("rows", "bf16", 512, 4097, kind="bwd_cap"))
    out.append(LnCase("rows", "f32", 512, 4097, kind="bwd_cap"))
    return out


def fwd_cap_case():
    return LnCase("rows", "bf16", 512, 262145, kind="fwd_cap")


def ids(cs):
    return [c.id for c in cs]


# ---------------------------------------------------------------------------------------------------------------- operands
def _rng(c: LnCase, salt: int):
    return np.random.default_rng(zlib.crc32(c.id.encode()) + salt)


@functools.lru_cache(maxsize=4)
def affine(c: LnCase):
    """integer gamma in {+-1, +-2} and beta in -3 .. 3 (None, None without affine)"""
    if not c.affine:
        return None, None
    g = _rng(c, 1)
    return g.choice([-2.0, -1.0, 1.0, 2.0], size=c.C), g.integers(-3, 4, size=c.C).astype(np.float64)


@functools.lru_cache(maxsize=4)
def exact_rows(c: LnCase) -> dict:
    """x, dy (rows, C) float64 with the expected y, dx, dgamma, dbeta, all exact; asserts the premises (see the module docstring)"""
    g = _rng(c, 2)
    R_, C = c.rows, c.C
    gamma, beta = affine(c)
    gam = gamma if gamma is not None else np.ones(C)
    bet = beta if beta is not None else np.zeros(C)
    a = 2.0 ** g.integers(0, 4, size=R_)
    mu = g.integers(-7, 8, size=R_).astype(np.float64)
    mu[np.abs(mu) == a] += 1.0                               # no x is 0: a lane step of zeros could leave a sum unnoticed
    if C == 1:
        x = mu[:, None].copy()
        dy = g.integers(-2, 3, size=(R_, 1)).astype(np.float64)
        return dict(x=x, dy=dy, eps=1e-5, y=np.broadcast_to(bet, (R_, 1)).copy(), dx=np.zeros((R_, 1)), dgamma=np.zeros(1), dbeta=dy.sum(0),
                    a=a, mu=mu, sigma=np.zeros((R_, 1)), m1=np.zeros(R_), m2=np.zeros(R_), g=dy * gam)
    assert C % 2 == 0
    base = np.where(np.arange(C) < C // 2, 1.0, -1.0)
    # +1 on one half of the row, -1 on the other, the row rolled by a whole number of lane steps and its sign drawn per row: every
    # lane step (64 channels, or the VEC channels of one lane of the rows form) is as unbalanced as it can be, so losing one from
    # a statistic moves the mean by a chunk / C
    steps = max(1, C // c.chunk)
    sigma = np.stack([g.choice([-1.0, 1.0]) * np.roll(base, c.chunk * int(g.integers(steps))) for _ in range(R_)])
    x = mu[:, None] + a[:, None] * sigma
    m1 = g.integers(-2, 3, size=R_).astype(np.float64)
    m2 = g.integers(-2, 3, size=R_).astype(np.float64)
    m2[m2 == 0] = 1.0                                        # every row can see a dropped m2
    h = np.zeros((R_, C))
    for r in range(R_):
        for s in (1.0, -1.0):
            idx = np.nonzero(sigma[r] == s)[0]
            n = len(idx) // 2
            t = g.integers(1, 4, size=n).astype(np.float64)
            h[r, idx[:n]], h[r, idx[n:2 * n]] = t, -t
    gg = 2.0 * (m1[:, None] + sigma * m2[:, None] + h)
    dy = gg / gam
    y = sigma * gam + bet
    dx = 2.0 * h / a[:, None]
    d = dict(x=x, dy=dy, eps=0.0, y=y, dx=dx, dgamma=(dy * sigma).sum(0), dbeta=dy.sum(0), a=a, mu=mu, sigma=sigma, m1=2 * m1, m2=2 * m2, g=gg)
    # ---- the premises, in numpy fp32
    f = np.float32
    assert np.array_equal(np.rint(dy), dy) and np.abs(dy).max() <= 14 and np.abs(x).max() <= 15
    for perm in (np.arange(C), g.permutation(C)):            # two summation orders
        xs = x.astype(f)[:, perm]
        s = np.zeros(R_, f)
        for k in range(C):
            s = s + xs[:, k]
        mean = s / f(C)
        assert np.array_equal(mean.astype(np.float64), mu)
        q = np.zeros(R_, f)
        for k in range(C):
            q = q + (xs[:, k] - mean) * (xs[:, k] - mean)
        var = q / f(C)
        assert np.array_equal(var.astype(np.float64), a * a)
        assert np.array_equal((f(1) / np.sqrt(var)).astype(np.float64), 1.0 / a)
    assert np.array_equal(gg.sum(1), C * d["m1"]) and np.array_equal((gg * sigma).sum(1), C * d["m2"])
    assert C * np.abs(gg).max() < 2 ** 24 and R_ * 14 < 2 ** 24
    for v in (x, dy, y, dx):                                 # numbers of both storage types
        assert np.abs(v).max() <= 256 and np.array_equal(store(v, "bf16"), v)
    return d


@functools.lru_cache(maxsize=4)
def general_rows(c: LnCase) -> dict:
    g = _rng(c, 3)
    x = g.integers(-3, 5, size=(c.rows, c.C)).astype(np.float64)
    dy = R.ternary((c.rows, c.C), 0.6, int(g.integers(1 << 30)), dtype=torch.float32).double().numpy()
    return dict(x=x, dy=dy, eps=1e-5)


def store(a: np.ndarray, dt: str) -> np.ndarray:
    f32 = np.ascontiguousarray(a, dtype=np.float64).astype(np.float32)
    if dt == "f32":
        return f32.astype(np.float64)
    return torch.from_numpy(f32).to(torch.bfloat16).to(torch.float64).numpy()


def to_storage(a: np.ndarray, dt: str) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(TORCH_DT[dt])


# ---------------------------------------------------------------------------------------------------------------- fp64 model
def model(c: LnCase, d: dict, defect=None, arg=None):
    """(y, dx) in fp64 from the LayerNorm formulas, with at most one defect of the kernels' index arithmetic"""
    x, dy, eps, C = d["x"], d["dy"], d["eps"], c.C
    gamma, beta = affine(c)
    gam = gamma if gamma is not None else np.ones(C)
    bet = beta if beta is not None else np.zeros(C)
    if defect == "neighbour_affine":
        gam, bet = np.roll(gam, -1), np.roll(bet, -1)
    keep_m = np.ones(C)
    keep_v = np.ones(C)
    if defect == "chunk_missing_mean":
        keep_m[arg * c.chunk:(arg + 1) * c.chunk] = 0
    if defect == "chunk_missing_var":
        keep_v[arg * c.chunk:(arg + 1) * c.chunk] = 0
    div = c.padded if defect == "padded_width" else C
    mean = (x * keep_m).sum(1, keepdims=True) / div
    var = (((x - mean) ** 2) * keep_v).sum(1, keepdims=True) / div
    with np.errstate(divide="ignore", invalid="ignore"):
        rstd = 1.0 / np.sqrt(var + eps)
    if defect == "neighbour_row_stats":
        mean, rstd = np.roll(mean, -1, axis=0), np.roll(rstd, -1, axis=0)
    with np.errstate(invalid="ignore"):
        xhat = (x - mean) * rstd
        y = xhat * gam + bet
        gg = dy * gam
        m1 = gg.sum(1, keepdims=True) / C
        m2 = (gg * xhat).sum(1, keepdims=True) / C
        if defect == "m2_dropped":
            m2 = 0 * m2
        dx = rstd * (gg - m1 - xhat * m2)
    if defect == "last_block_skipped":
        for out, bwd in ((y, False), (dx, True)):
            b = c.block_rows(bwd)
            out[(c.rows // b) * b:] = np.nan
    return y, dx


def defects(c: LnCase):
    out = []
    if c.C > 1:
        nchunk = -(-c.C // c.chunk)
        if nchunk > 1:
            out += [(n, k) for n in ("chunk_missing_mean", "chunk_missing_var") for k in sorted({0, nchunk - 1})]
        out.append(("m2_dropped", None))
        if c.rows > 1:
            out.append(("neighbour_row_stats", None))
    if c.padded != c.C:
        out.append(("padded_width", None))
    if c.affine and c.C > 1:
        out.append(("neighbour_affine", None))
    if c.rows % c.block_rows(False) or c.rows % c.block_rows(True):
        out.append(("last_block_skipped", None))
    return out


def rsqrt_bound(c: LnCase, d: dict):
    """(bound_y, bound_dx) per element for the exact rows on a device whose rsqrtf is not exact at 4^k: the module docstring"""
    gamma, _ = affine(c)
    gam = np.abs(gamma) if gamma is not None else np.ones(c.C)
    by = 2 * U * (4 * gam[None, :] + np.abs(d["y"]))
    sg = np.abs(d["g"]).sum(1, keepdims=True)
    e2 = (c.C / 64 + 11) * U * sg / c.C
    m1, m2 = np.abs(d["m1"])[:, None], np.abs(d["m2"])[:, None]
    bdx = 2 * (e2 + 3 * U * m2 + 6 * U * (np.abs(d["g"]) + m1 + m2)) / d["a"][:, None]
    return by, np.broadcast_to(bdx, d["dx"].shape)


def general_bounds(c: LnCase, d: dict):
    """fp64 (y, dx) of the general rows and the per-element bounds |kernel - fp64| <= (By, Bdx), first order in u = 2^-24 and doubled
    for the second-order terms, counting the kernels' fp32 operations (n = c.n_seq sequential additions per lane, a 6-step tree):
      mean: the sum of integers is exact, the division rounds: e_mean = u |mean|;   dc = x - mean: e_d = e_mean + u |dc|
      q = sum dc^2: e_q = sum(2 |dc| e_d + u dc^2) + (n + 6) u q;  var = q / C (+ u), + eps (+ u): rel_v = e_q / (q + C eps) + 2 u
      rstd: 1 ulp reciprocal square root (2 u), or sqrt and divide (2 u): rel_r = rel_v / 2 + 2 u
      xhat = dc rstd: e_x = e_d rstd + |xhat| (rel_r + u);   y = xhat gamma + beta: By = |gamma| e_x + u |xhat gamma| + u |y|
      m1 = sum g / C, g integers: u |m1|;  s2 = sum g xhat: e_s2 = sum |g| (e_x + u |xhat|) + (n + 6) u sum |g xhat|;
      m2 = s2 / C: e_m2 = e_s2 / C + u |m2|
      inner = g - m1 - xhat m2: e_in = u |m1| + e_x |m2| + |xhat| e_m2 + u |xhat m2| + 2 u (|g| + |m1| + |xhat m2|)
      dx = rstd inner: Bdx = rstd e_in + |dx| (rel_r + u)
    plus half an ulp of the storage type: u |ref| (fp32, 24 significant bits), 2^-8 |ref| (bf16, 8 significant bits)."""
    x, dy, eps, C = d["x"], d["dy"], d["eps"], c.C
    gamma, beta = affine(c)
    gam = gamma if gamma is not None else np.ones(C)
    bet = beta if beta is not None else np.zeros(C)
    y, dx = model(c, d)
    n = c.n_seq
    mean = x.mean(1, keepdims=True)
    dc = x - mean
    e_d = U * np.abs(mean) + U * np.abs(dc)
    q = (dc ** 2).sum(1, keepdims=True)
    e_q = (2 * np.abs(dc) * e_d + U * dc ** 2).sum(1, keepdims=True) + (n + 6) * U * q
    rel_v = e_q / (q + C * eps) + 2 * U
    rel_r = rel_v / 2 + 2 * U
    rstd = 1 / np.sqrt(q / C + eps)
    xhat = dc * rstd
    e_x = e_d * rstd + np.abs(xhat) * (rel_r + U)
    By = np.abs(gam) * e_x + U * np.abs(xhat * gam) + U * np.abs(y)
    gg = dy * gam
    m1 = gg.sum(1, keepdims=True) / C
    m2 = (gg * xhat).sum(1, keepdims=True) / C
    e_s2 = (np.abs(gg) * (e_x + U * np.abs(xhat))).sum(1, keepdims=True) + (n + 6) * U * np.abs(gg * xhat).sum(1, keepdims=True)
    e_m2 = e_s2 / C + U * np.abs(m2)
    e_in = U * np.abs(m1) + e_x * np.abs(m2) + np.abs(xhat) * e_m2 + U * np.abs(xhat * m2) + 2 * U * (np.abs(gg) + np.abs(m1) + np.abs(xhat * m2))
    Bdx = rstd * e_in + np.abs(dx) * (rel_r + U)
    half = U if c.dt == "f32" else 2.0 ** -8           # half an ulp of an 8-bit significand, relative to |ref|
    return y, dx, 2 * By + half * np.abs(y), 2 * Bdx + half * np.abs(dx)


def discrimination(c: LnCase) -> dict:
    """per defect: (largest change of a stored output of the exact rows, that change over the largest rsqrt bound)"""
    d = exact_rows(c)
    y0, dx0 = model(c, d)
    assert np.array_equal(y0, d["y"]) and np.array_equal(dx0, d["dx"]), f"{c.id}: the fp64 formulas do not give the closed form"
    by, bdx = rsqrt_bound(c, d)
    bound = max(float(by.max()), float(bdx.max()))
    out = {}
    for name, arg in defects(c):
        y, dx = model(c, d, name, arg)
        ch = 0.0
        for got, ref in ((y, y0), (dx, dx0)):
            diff = np.where(np.isnan(got), np.inf, np.abs(got - ref))
            ch = max(ch, float(diff.max()))
        out[(name, arg)] = (ch, ch / bound)
    return out

"""Exact-arithmetic cases for the decoder joins of the MONAI models: UpCat ([skip, up], replicate-padded to the skip's grid) and the
deconv-first placement ([up, skip]) of csrc/upcat_kernels.hip -- upcat_gemm_kernel<T, FWD | DGRAD> and upcat_copy_channels_kernel.

The operands are ternary activations, gradients and weights and an integer bias: every product is an integer and the sum of the
magnitudes of one output's terms stays far below 2^24, so the fp32 MFMA accumulation is the fp64 sum in whatever order the k steps
run, adding the bias is exact, and the ONE rounding is the store.  For the bf16 cases |reference| <= 256, so the store is exact too;
three special kinds leave that range on purpose:
  round    the forward stores 257, 259, 261 as 256, 260, 260 (a truncating store: 256, 258, 260), and the data gradient folds eight
           face terms into G' = 259, which the bf16 route rounds to 260 BEFORE the MFMA (so dx_low = 260 - 256 = 4, not 3);
  wconv    fp32 weights 1 + j 2^-10, j in {3, 4, 5, 12}: the bf16 route stages them as 1, 1, 1 + 2^-7, 1 + 2^-6 (ties to even; a
           truncating conversion gives 1, 1, 1, 1 + 2^-7), products are multiples of 2^-7;
  copycap  a skip of 33 x 65 x 65 x 16 elements, more than the 8192 x 256 threads of the copy grid: a second grid-stride trip.

The module restates the launch rules it relies on (tile 64 x 64, k step 32 / 16, the copy cap, the row-tile limit of gridDim.y);
tests/test_host_decoder_exact_cases.py checks each against the launch code, proves the premises on the CPU and shows that every defect
of its list changes a stored output of every case it applies to.  Two computations of the expected tensors exist on purpose: a torch
fp64 conv_transpose3d + replicate pad + cat with autograd (the operation as MONAI states it), and a numpy model of the kernel's index
arithmetic (row -> voxel, parity -> offset, face flags) that can be evaluated with one defect at a time.  They must agree.

Plain module (no tests)."""
from __future__ import annotations

import functools
import itertools
import zlib
from dataclasses import dataclass

import numpy as np
import torch

import exact_reduction_cases as R

TORCH_DT = {"bf16": torch.bfloat16, "f32": torch.float32}

# ---- launch rules of csrc/upcat_kernels.hip, restated (test_host_decoder_exact_cases.py reads them out of the source)
UP_BP = UP_BQ = 64                       # one workgroup: 64 P (columns) x 64 Q (low-resolution rows), four waves of 32 x 32
KSTEP = {"bf16": 32, "f32": 16}          # k per staging step
COPY_BLOCK, COPY_MAX_BLOCKS = 256, 8192  # upcat_copy_channels_kernel: grid-stride past 8192 blocks of 256
MAX_ROW_TILES = 65535                    # row tiles sit on gridDim.y; more are refused by name

BF16_INT_CAP = 256                       # every integer up to here is a bf16 number


def gemm_dims(c: "UpCase", mode: str):
    """(P, Q, K) of the forward / data-gradient GEMM"""
    C_in, _, C_u = c.ch
    return (8 * C_u, c.rows, C_in) if mode == "fwd" else (C_in, c.rows, 8 * C_u)


def gemm_grid(c: "UpCase", mode: str):
    P, Q, _ = gemm_dims(c, mode)
    return (-(-P // UP_BP), -(-Q // UP_BQ))


def k_steps(c: "UpCase", mode: str) -> int:
    return -(-gemm_dims(c, mode)[2] // KSTEP[c.dt])


def copy_trips(elements: int) -> int:
    """grid-stride trips of the longest-running thread of upcat_copy_channels_kernel"""
    blocks = min(-(-elements // COPY_BLOCK), COPY_MAX_BLOCKS)
    return -(-elements // (blocks * COPY_BLOCK)) if elements else 0


def refused_rows(rows: int) -> bool:
    return -(-rows // UP_BQ) > MAX_ROW_TILES


# ---------------------------------------------------------------------------------------------------------------- the cases
@dataclass(frozen=True)
class UpCase:
    place: str                # "upcat": [skip, up], skip grid 2 low + odd; "upfirst": [up, skip], skip grid exactly 2 low
    dt: str                   # "bf16" | "f32"
    ch: tuple                 # (C_in, C_e, C_u)
    low: tuple                # low-resolution grid (d, h, w)
    odd: tuple = (0, 0, 0)    # per axis: skip = 2 low + odd
    N: int = 1
    kind: str = "ternary"     # ternary | round | wconv | copycap
    bias: bool = True

    @property
    def skip(self):
        return tuple(2 * l + o for l, o in zip(self.low, self.odd))

    @property
    def rows(self):
        return self.N * self.low[0] * self.low[1] * self.low[2]

    @property
    def Ct(self):
        return self.ch[1] + self.ch[2]

    @property
    def up_off(self):
        return self.ch[1] if self.place == "upcat" else 0

    @property
    def skip_off(self):
        return 0 if self.place == "upcat" else self.ch[2]

    @property
    def other_up_off(self):
        """the up half's offset under the OTHER placement"""
        return 0 if self.place == "upcat" else self.ch[1]

    @property
    def straddles(self) -> bool:
        """some 64-row tile holds rows of two samples"""
        per = self.rows // self.N
        return self.N > 1 and per % UP_BQ != 0

    @property
    def id(self):
        ci, ce, cu = self.ch
        g = "x".join(map(str, self.low))
        o = "".join(map(str, self.odd))
        return f"{self.place}-{self.kind}-{self.dt}-c{ci}_{ce}_{cu}-low{g}-odd{o}-n{self.N}" + ("" if self.bias else "-nobias")


CHANNELS = ((3, 7, 5), (16, 1, 8), (33, 4, 12), (72, 32, 24), (130, 8, 9))
ODD8 = tuple(itertools.product((0, 1), repeat=3))


def upcat_cases():
    out = []
    for dt in ("bf16", "f32"):
        for ch in CHANNELS:
            out.append(UpCase("upcat", dt, ch, (1, 1, 1), (1, 1, 1), 1))
            out.extend(UpCase("upcat", dt, ch, (2, 3, 5), odd, 1, bias=odd != (0, 1, 0)) for odd in ODD8)
            out.append(UpCase("upcat", dt, ch, (3, 4, 6), (1, 0, 1), 3))
    return out


def upfirst_cases():
    out = []
    for dt in ("bf16", "f32"):
        for ch in CHANNELS + ((33, 0, 12),):
            out.append(UpCase("upfirst", dt, ch, (1, 1, 1), N=1))
            out.append(UpCase("upfirst", dt, ch, (2, 3, 5), N=1, bias=ch[0] != 16))
            out.append(UpCase("upfirst", dt, ch, (3, 4, 6), N=3))
    return out


def special_cases():
    return [
        UpCase("upcat", "bf16", (16, 1, 3), (1, 1, 1), (1, 1, 1), 1, kind="round"),
        UpCase("upcat", "bf16", (16, 1, 8), (2, 3, 5), (1, 0, 1), 1, kind="wconv", bias=False),
        UpCase("upfirst", "bf16", (16, 1, 8), (2, 3, 5), N=1, kind="wconv", bias=False),
        UpCase("upcat", "bf16", (8, 16, 8), (16, 32, 32), (1, 1, 1), 1, kind="copycap"),
    ]


def all_cases():
    return upcat_cases() + upfirst_cases() + special_cases()


def ids(cs):
    return [c.id for c in cs]


# ---------------------------------------------------------------------------------------------------------------- operands
WCONV_J = (3, 4, 5, 12)
WCONV_STAGED = {3: 1.0, 4: 1.0, 5: 1.0 + 2.0 ** -7, 12: 1.0 + 2.0 ** -6}        # round to nearest even into bf16
WCONV_TRUNCATED = {3: 1.0, 4: 1.0, 5: 1.0, 12: 1.0 + 2.0 ** -7}


def _np(t: torch.Tensor) -> np.ndarray:
    return t.to(torch.float64).numpy()


def _quarters(shape, seed):
    """k / 4, |k| <= 127: numbers of both storage types, varied enough that a misplaced copy shows"""
    rng = np.random.default_rng(seed)
    return rng.integers(-127, 128, size=shape).astype(np.float64) / 4.0


@functools.lru_cache(maxsize=8)
def operands(c: UpCase) -> dict:
    """float64 numpy operands, every value a number of the case's storage type (weights and bias: fp32): x (N, d, h, w, C_in),
    w (C_in, C_u, 2, 2, 2), bias (C_u) | None, xe (N, D, H, W, C_e) | None, dcat (N, D, H, W, C_e + C_u)"""
    C_in, C_e, C_u = c.ch
    seed = zlib.crc32(c.id.encode())
    N, low, skip = c.N, c.low, c.skip
    if c.kind == "round":
        x = np.full((N, *low, C_in), 16.0)
        w = np.ones((C_in, C_u, 2, 2, 2))
        bias = np.array([1.0, 3.0, 5.0])
        dcat = np.zeros((N, *skip, c.Ct))
        up = dcat[..., c.up_off:]
        up[0, 1, 1, 1, 0] = 256.0                         # parity 7's child, and three of the seven faces replicated from it
        up[0, 2, 1, 1, 0] = up[0, 1, 2, 1, 0] = up[0, 1, 1, 2, 0] = 1.0
        up[0, 1, 1, 1, 1] = -256.0
    else:
        dx, dw, dg = {"ternary": (0.6, 0.6, 0.5), "copycap": (0.6, 0.6, 0.5), "wconv": (0.1, 1.0, 0.04)}[c.kind]
        if c.kind == "ternary" and (c.rows == 1 or C_in < 16):
            # one row, or three input channels: a zero would leave an input channel or a k index without any term in the whole
            # case, so nothing is zero (the single row's gradients are 1 or 2 as well: a folded face sum cannot cancel)
            dx = dw = 1.0
        x = _np(R.ternary((N, *low, C_in), dx, seed, dtype=torch.float32))
        if c.kind == "wconv":
            i, o, p = np.meshgrid(np.arange(C_in), np.arange(C_u), np.arange(8), indexing="ij")
            j = np.array(WCONV_J)[(i + 2 * o + 3 * p) % 4]
            w = (1.0 + j * 2.0 ** -10).reshape(C_in, C_u, 2, 2, 2)
        else:
            w = _np(R.ternary((C_in, C_u, 2, 2, 2), dw, seed + 1, dtype=torch.float32))
        bias = np.random.default_rng(seed + 2).integers(-3, 4, size=C_u).astype(np.float64) if c.bias else None
        dcat = np.empty((N, *skip, c.Ct))
        dcat[..., c.up_off:c.up_off + C_u] = _np(R.ternary((N, *skip, C_u), dg, seed + 3, dtype=torch.float32))
        if c.kind == "ternary" and c.rows == 1:
            dcat[..., c.up_off:c.up_off + C_u] = np.random.default_rng(seed + 7).integers(1, 3, size=(N, *skip, C_u))
        if C_e:
            dcat[..., c.skip_off:c.skip_off + C_e] = _quarters((N, *skip, C_e), seed + 4)
    xe = _quarters((N, *skip, C_e), seed + 5) if C_e else None
    return dict(x=x, w=w, bias=bias, xe=xe, dcat=dcat)


# ---------------------------------------------------------------------------------------------------------------- roundings
def store(a: np.ndarray, dt: str, trunc: bool = False) -> np.ndarray:
    """a (float64) as the kernel stores it -- once to fp32 (exact on these cases: premises()), once to the storage type -- as float64"""
    f32 = np.ascontiguousarray(a, dtype=np.float64).astype(np.float32)
    if dt == "f32":
        return f32.astype(np.float64)
    if trunc:
        return (f32.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)
    return torch.from_numpy(f32).to(torch.bfloat16).to(torch.float64).numpy()


def staged_weight(c: UpCase, w: np.ndarray, trunc: bool = False) -> np.ndarray:
    """the fp32 weight as the MFMA sees it: rounded to bf16 when staged on the bf16 route"""
    return store(w, c.dt, trunc)


# ---------------------------------------------------------------------------------------------------------------- index model
def _coords(c: UpCase, sample0: bool = False):
    d, h, w = c.low
    r = np.arange(c.rows)
    x, y, z, n = r % w, r // w % h, r // (w * h) % d, r // (w * h * d)
    if sample0:                                        # defect: a tile takes the sample of its first row
        n = n[(r // UP_BQ) * UP_BQ]
    fz = (z == d - 1) & bool(c.odd[0])
    fy = (y == h - 1) & bool(c.odd[1])
    fx = (x == w - 1) & bool(c.odd[2])
    return n, z, y, x, (fz, fy, fx)


def _targets(c: UpCase, defect=None):
    """for every parity and face copy: (parity, is a face copy, per-axis copy flags, row mask, voxel index arrays)"""
    n, z, y, x, (fz, fy, fx) = _coords(c, sample0=defect == "row_info_sample0")
    for par in range(8):
        a, b, cc = par >> 2, (par >> 1) & 1, par & 1
        if defect == "parity_perm":
            a, cc = cc, a
        ez, ey, ex = fz & bool(a), fy & bool(b), fx & bool(cc)
        for zz, yy, xx in ODD8:
            m = (ez | (zz == 0)) & (ey | (yy == 0)) & (ex | (xx == 0))
            if m.any():
                yield par, (zz, yy, xx), m, (n[m], 2 * z[m] + a + zz, 2 * y[m] + b + yy, 2 * x[m] + cc + xx)


def fwd_values(c: UpCase, defect=None, arg=None) -> np.ndarray:
    """stored values (rows, 8, C_u) of the up half before the scatter"""
    d = operands(c)
    C_in, _, C_u = c.ch
    x = d["x"].reshape(c.rows, C_in).copy()
    wq = staged_weight(c, d["w"].reshape(C_in, C_u, 8), trunc=defect == "trunc_weight")
    if defect == "drop_k_step":
        x[:, arg * KSTEP[c.dt]:(arg + 1) * KSTEP[c.dt]] = 0
    elif defect == "drop_channel":
        x[:, arg] = 0
    G = np.einsum("ri,iop->rpo", x, wq)
    if d["bias"] is not None:
        G = G + (d["bias"][np.arange(8) % C_u][None, :, None] if defect == "bias_par" else d["bias"][None, None, :])
    return store(G, c.dt, trunc=defect == "trunc_store")


def fwd_model(c: UpCase, defect=None, arg=None) -> np.ndarray:
    """the concat buffer (N, D, H, W, C_e + C_u) as stored, float64; NaN where nothing is written"""
    d = operands(c)
    _, C_e, C_u = c.ch
    val = fwd_values(c, defect, arg)
    out = np.full((c.N, *c.skip, c.Ct), np.nan)
    if C_e:
        out[..., c.skip_off:c.skip_off + C_e] = d["xe"]
        if defect == "copy_one_trip":
            flat = out[..., c.skip_off:c.skip_off + C_e].reshape(-1).copy()
            flat[COPY_MAX_BLOCKS * COPY_BLOCK:] = np.nan
            out[..., c.skip_off:c.skip_off + C_e] = flat.reshape(c.N, *c.skip, C_e)
    uo = c.other_up_off if defect == "up_off_other" else c.up_off
    for par, copy, m, (n, Z, Y, X) in _targets(c, defect):
        if defect == "face_unwritten" and copy[arg]:
            continue
        out[n, Z, Y, X, uo:uo + C_u] = val[m, par, :]
    if defect == "face_from_2d-2":                     # the replicated plane 2d of axis `arg` copies plane 2d - 2
        sl_dst = [slice(None)] * 5
        sl_src = [slice(None)] * 5
        sl_dst[1 + arg], sl_src[1 + arg] = 2 * c.low[arg], 2 * c.low[arg] - 2
        sl_dst[4] = sl_src[4] = slice(uo, uo + C_u)
        out[tuple(sl_dst)] = out[tuple(sl_src)]
    return out


def dgrad_values(c: UpCase, defect=None, arg=None) -> np.ndarray:
    """G' (rows, 8, C_u): the child's gradient plus the faces replicated from it, as the MFMA sees it"""
    g = operands(c)["dcat"]
    C_u = c.ch[2]
    uo = c.other_up_off if defect == "up_off_other" else c.up_off
    Gp = np.zeros((c.rows, 8, C_u))
    for par, copy, m, (n, Z, Y, X) in _targets(c, defect):
        mult = 1.0
        if any(copy):
            if defect == "fold_missing":
                continue
            if defect == "fold_twice":
                mult = 2.0
        Gp[m, par, :] += mult * g[n, Z, Y, X, uo:uo + C_u]
    if defect != "gp_unrounded":
        Gp = store(Gp, c.dt)
    flat = Gp.reshape(c.rows, 8 * C_u)
    if defect == "drop_k_step":
        flat[:, arg * KSTEP[c.dt]:(arg + 1) * KSTEP[c.dt]] = 0
    elif defect == "drop_channel":
        flat[:, arg] = 0
    return Gp


def dgrad_model(c: UpCase, defect=None, arg=None):
    """(dx_e (N, D, H, W, C_e) | None, dx_low (N, d, h, w, C_in)) as stored, float64"""
    d = operands(c)
    C_in, C_e, C_u = c.ch
    wq = staged_weight(c, d["w"].reshape(C_in, C_u, 8), trunc=defect == "trunc_weight")
    dx = np.einsum("rpo,iop->ri", dgrad_values(c, defect, arg), wq)
    dx_low = store(dx, c.dt, trunc=defect == "trunc_store").reshape(c.N, *c.low, C_in)
    dx_e = None
    if C_e:
        dx_e = d["dcat"][..., c.skip_off:c.skip_off + C_e].copy()
        if defect == "copy_one_trip":
            flat = dx_e.reshape(-1)
            flat[COPY_MAX_BLOCKS * COPY_BLOCK:] = np.nan
    return dx_e, dx_low


# ---------------------------------------------------------------------------------------------------------------- fp64 reference
def reference(c: UpCase):
    """The operation as MONAI states it, in fp64 with the staged weights: cat (N, D, H, W, Ct), and by autograd of <dcat, cat> the
    gradients dx_e, dx_low -- before any storage rounding (and without the bf16 rounding of G': see premises)."""
    d = operands(c)
    C_in, C_e, C_u = c.ch
    cf = lambda a: torch.from_numpy(np.ascontiguousarray(a)).permute(0, 4, 1, 2, 3)
    x = cf(d["x"]).clone().requires_grad_(True)
    w = torch.from_numpy(staged_weight(c, d["w"]))
    b = torch.from_numpy(d["bias"]) if d["bias"] is not None else None
    up = torch.nn.functional.conv_transpose3d(x, w, b, stride=2)
    if any(c.odd):
        up = torch.nn.functional.pad(up, (0, c.odd[2], 0, c.odd[1], 0, c.odd[0]), mode="replicate")
    parts = [up]
    xe = None
    if C_e:
        xe = cf(d["xe"]).clone().requires_grad_(True)
        parts = [xe, up] if c.place == "upcat" else [up, xe]
    cat = torch.cat(parts, 1)
    (cat * cf(d["dcat"])).sum().backward()
    last = lambda t: t.detach().permute(0, 2, 3, 4, 1).contiguous().numpy()
    return last(cat), (last(xe.grad) if C_e else None), last(x.grad)


def _same(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=True))


def changed(a: np.ndarray, b: np.ndarray) -> int:
    """stored outputs that differ (NaN = unwritten counts as a value)"""
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())


@functools.lru_cache(maxsize=8)
def premises(c: UpCase) -> dict:
    """Asserts, for the reference alone, that the case is exact, and returns the expected stored tensors (float64) with the facts:
    - every operand is a number of its type; every term of an output is a multiple of one unit with sum|terms| < 2^24 units
      (assert_exact_cap), so the fp32 accumulator holds the fp64 sum and the store is the only rounding;
    - bf16, kind ternary / copycap: |reference| <= 256 and integer, so the store is exact as well;
    - the index model without a defect IS the fp64 reference rounded once to storage."""
    d = operands(c)
    C_in, C_e, C_u = c.ch
    bf = c.dt == "bf16"
    for k in ("x", "xe", "dcat"):
        if d[k] is not None:
            assert _same(store(d[k], c.dt), d[k]), f"{c.id}: {k} holds values that are no {c.dt} numbers"
    assert _same(store(d["w"], "f32"), d["w"]) and (d["bias"] is None or _same(store(d["bias"], "f32"), d["bias"]))
    unit = 2.0 ** -7 if c.kind == "wconv" else 1.0
    wq = np.abs(staged_weight(c, d["w"].reshape(C_in, C_u, 8)))
    fwd_abs = float(np.einsum("ri,iop->rpo", np.abs(d["x"].reshape(c.rows, C_in)), wq).max())
    fwd_abs += float(np.abs(d["bias"]).max()) if d["bias"] is not None else 0.0
    R.assert_exact_cap(fwd_abs, unit, what=f"{c.id} forward")
    gp_raw = dgrad_values(c, "gp_unrounded")
    gp = dgrad_values(c)
    if c.kind != "round":
        assert _same(gp, gp_raw), f"{c.id}: a folded face sum is no {c.dt} number"
    dg_abs = float(np.einsum("rpo,iop->ri", np.abs(gp), wq).max())
    R.assert_exact_cap(dg_abs, unit, what=f"{c.id} data gradient")

    cat64, dxe64, dxl64 = reference(c)
    for a in (cat64, dxl64):
        assert _same(a.astype(np.float32).astype(np.float64), a), f"{c.id}: the reference is no fp32 number"
    cat, (dx_e, dx_low) = fwd_model(c), dgrad_model(c)
    assert not np.isnan(cat).any() and not np.isnan(dx_low).any()
    assert _same(cat, store(cat64, c.dt)), f"{c.id}: the index model and the fp64 reference differ (forward)"
    if C_e:
        assert _same(dx_e, dxe64)
        assert _same(cat[..., c.skip_off:c.skip_off + C_e], d["xe"])
    if c.kind != "round":
        assert _same(dx_low, store(dxl64, c.dt)), f"{c.id}: the index model and the fp64 reference differ (data gradient)"
    if bf and c.kind in ("ternary", "copycap"):
        for a, a64 in ((cat[..., c.up_off:c.up_off + C_u], cat64[..., c.up_off:c.up_off + C_u]), (dx_low, dxl64)):
            assert float(np.abs(a64).max()) <= BF16_INT_CAP and _same(a, a64), f"{c.id}: |reference| over {BF16_INT_CAP} in bf16"
    if c.kind == "round":
        u = cat[0, :, :, :, c.up_off:]
        assert (u == np.array([256.0, 260.0, 260.0])).all()
        assert (store(cat64, c.dt, trunc=True)[0, 0, 0, 0, c.up_off:] == np.array([256.0, 258.0, 260.0])).all()
        assert (dx_low == 4.0).all() and (dxl64 == 3.0).all()              # G' = 259 is staged as 260
    if c.kind == "wconv":
        j = np.rint((d["w"] - 1.0) * 2.0 ** 10).astype(int)
        for jj in WCONV_J:
            assert (staged_weight(c, d["w"])[j == jj] == WCONV_STAGED[jj]).all() and (j == jj).any()
            assert (staged_weight(c, d["w"], trunc=True)[j == jj] == WCONV_TRUNCATED[jj]).all()
    for axis in range(3):                                                  # a replicated face is the plane it copies
        if c.odd[axis]:
            up = np.moveaxis(cat[..., c.up_off:c.up_off + C_u], 1 + axis, 0)
            assert _same(up[2 * c.low[axis]], up[2 * c.low[axis] - 1])
    return dict(cat=cat, dx_e=dx_e, dx_low=dx_low, fwd_abs=fwd_abs, dgrad_abs=dg_abs, unit=unit)


def to_storage(a: np.ndarray, dt: str) -> torch.Tensor:
    """a float64 array of storage-type numbers as a tensor of that type"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(TORCH_DT[dt])


# ---------------------------------------------------------------------------------------------------------------- defects
def defects(c: UpCase):
    """[(pass, defect, arg)] that apply to the case: each is one in-bounds change of the kernel's arithmetic or indexing"""
    C_in, C_e, C_u = c.ch
    out = []
    if c.kind == "round":         # constant operands: the case is there for the two roundings (and cannot tell parities apart)
        return [("fwd", "trunc_store", None), ("dgrad", "gp_unrounded", None), ("fwd", "drop_k_step", 0), ("dgrad", "drop_k_step", 0)]
    if c.kind == "wconv":         # sparse operands keep the sums small enough for 2^-7 to survive the store: the conversion alone
        return [(m, n, None) for m in ("fwd", "dgrad") for n in ("trunc_weight", "parity_perm")]
    for mode in ("fwd", "dgrad"):
        out += [(mode, "drop_k_step", s) for s in range(k_steps(c, mode))]
        out += [(mode, "parity_perm", None)]
        if C_e:
            out.append((mode, "up_off_other", None))
        if c.straddles:
            out.append((mode, "row_info_sample0", None))
        if c.kind == "copycap":
            out.append((mode, "copy_one_trip", None))
    for axis in range(3):
        if c.odd[axis]:
            out += [("fwd", "face_from_2d-2", axis), ("fwd", "face_unwritten", axis)]
    if any(c.odd):
        out += [("dgrad", "fold_missing", None), ("dgrad", "fold_twice", None)]
    if c.bias and C_u > 1:
        out.append(("fwd", "bias_par", None))
    return out


def discrimination(c: UpCase) -> dict:
    """{(pass, defect, arg): stored outputs the defect changes}; plus, per pass, the input channels / k indices whose loss changes
    nothing (must be empty: checked on the values before the scatter, which is one-to-one onto the written elements, by taking the
    channel's terms out of the unrounded sums and storing again)"""
    ref = premises(c)
    found = {}
    for mode, name, arg in defects(c):
        if mode == "fwd":
            found[(mode, name, arg)] = changed(fwd_model(c, name, arg), ref["cat"])
        else:
            dx_e, dx_low = dgrad_model(c, name, arg)
            found[(mode, name, arg)] = changed(dx_low, ref["dx_low"]) + (changed(dx_e, ref["dx_e"]) if dx_e is not None else 0)
    if c.kind == "ternary":
        d = operands(c)
        C_in, _, C_u = c.ch
        wq = staged_weight(c, d["w"].reshape(C_in, C_u, 8))
        x = d["x"].reshape(c.rows, C_in)
        pre = np.einsum("ri,iop->rpo", x, wq) + (d["bias"][None, None, :] if d["bias"] is not None else 0.0)
        kept = store(pre, c.dt)
        found[("fwd", "silent_channels", None)] = [
            i for i in range(C_in) if not changed(store(pre - x[:, i, None, None] * wq[i].T[None], c.dt), kept)]
        gp = dgrad_values(c).reshape(c.rows, -1)
        wk = wq.transpose(2, 1, 0).reshape(8 * C_u, C_in)                  # k = par * C_u + o
        pre = gp @ wk
        kept = store(pre, c.dt)
        found[("dgrad", "silent_channels", None)] = [
            k for k in range(8 * C_u) if not changed(store(pre - gp[:, k, None] * wk[None, k], c.dt), kept)]
    return found


# =====================================================================================================================
# B. thin transposed convs: ConvTranspose3d(k 3, s 2, p 1, output padding 1) with C_out <= 4 (csrc/conv3d_strided_kernels.hip)
# convT3d_thin_kernel (a thread per output voxel, grid-stride past 65536 blocks) and, for ONE output channel through hip_ops,
# convT3d_c1_dots_kernel + convT3d_c1_gather_kernel.  x ternary, w ternary (fp32, never rounded: it sits in LDS as fp32), integer
# bias: every fmaf is exact, so both routes give the fp64 sum, and for bf16 |reference| <= 256 makes the store exact.
# =====================================================================================================================
THIN_OMAX = 4
THIN_LDS_BYTES = 64 * 1024
THIN_MAX_BLOCKS, THIN_BLOCK = 65536, 256
C1_MAX_CIN = 512                          # hip_ops routes C_out = 1 to the dots + gather pair up to here


def thin_supported(c_in: int, c_out: int) -> bool:
    return 1 <= c_out <= THIN_OMAX and c_in >= 8 and c_in % 8 == 0 and 27 * c_out * c_in * 4 <= THIN_LDS_BYTES


def thin_routes(c_in: int, c_out: int):
    """the kernels that compute a (C_in, C_out) layer: through hip_ops, and through pytc_convT3d_thin_fwd directly"""
    via_ops = "c1" if c_out == 1 and c_in % 8 == 0 and c_in <= C1_MAX_CIN else "thin"
    return via_ops, "thin"


def thin_trips(outputs: int) -> int:
    blocks = min(-(-outputs // THIN_BLOCK), THIN_MAX_BLOCKS)
    return -(-outputs // (blocks * THIN_BLOCK))


@dataclass(frozen=True)
class ThinCase:
    dt: str
    cin: int
    cout: int
    grid: tuple               # input grid
    N: int
    bias: bool
    kind: str = "ternary"     # ternary | round | cap

    @property
    def out_grid(self):
        return tuple(2 * g for g in self.grid)

    @property
    def outputs(self):
        return self.N * 8 * self.grid[0] * self.grid[1] * self.grid[2]

    @property
    def id(self):
        return (f"thin-{self.kind}-{self.dt}-c{self.cin}_{self.cout}-in{'x'.join(map(str, self.grid))}-n{self.N}"
                + ("" if self.bias else "-nobias"))


THIN_CHANNELS = tuple((ci, co) for ci in (8, 24, 64) for co in (1, 2, 3, 4)) + ((512, 1),)
THIN_GRIDS = ((1, 1, 1), (1, 2, 3), (3, 4, 5))


def thin_cases():
    out = []
    for dt in ("bf16", "f32"):
        for k, (ci, co) in enumerate(THIN_CHANNELS):
            for j, g in enumerate(THIN_GRIDS):
                flip = (k + j) % 2 == 0                     # N in {1, 3} and bias on / off, each with each over the table
                out.append(ThinCase(dt, ci, co, g, 1, flip))
                out.append(ThinCase(dt, ci, co, g, 3, not flip))
    out.append(ThinCase("bf16", 8, 3, (1, 1, 1), 1, True, kind="round"))
    return out


def thin_cap_case():
    return ThinCase("bf16", 8, 1, (64, 64, 65), 8, True, kind="cap")


@functools.lru_cache(maxsize=4)
def thin_operands(c: ThinCase) -> dict:
    """float64: x (N, D, H, W, C_in), w (C_in, C_out, 3, 3, 3), bias (C_out) | None"""
    seed = zlib.crc32(c.id.encode())
    if c.kind == "round":              # every output voxel of a one-voxel input sees ONE tap: 8 x 16 x 2 = 256, + 1, 3, 5
        return dict(x=np.full((1, 1, 1, 1, 8), 16.0), w=np.full((8, 3, 3, 3, 3), 2.0), bias=np.array([1.0, 3.0, 5.0]))
    if c.kind == "cap":
        # closed form: only input channel 5 has weights (27 integer taps), so the output is the one-channel transposed conv of that
        # channel's ternary field; the other channels carry ternary values against zero weights
        x = _np(R.ternary((c.N, *c.grid, c.cin), 0.5, seed, dtype=torch.float32))
        w = np.zeros((c.cin, 1, 27))
        w[5, 0] = np.arange(27) % 7 - 3.0
        return dict(x=x, w=w.reshape(c.cin, 1, 3, 3, 3), bias=np.array([2.0]))
    # a one-voxel input has no second voxel to give a channel chunk a term: nothing is zero there
    dens = 1.0 if c.grid == (1, 1, 1) else (0.5 if c.cin <= 64 else 0.25)
    x = _np(R.ternary((c.N, *c.grid, c.cin), dens, seed, dtype=torch.float32))
    w = _np(R.ternary((c.cin, c.cout, 3, 3, 3), 1.0 if c.cin <= 24 or c.grid == (1, 1, 1) else 0.5, seed + 1, dtype=torch.float32))
    bias = (np.random.default_rng(seed + 2).permutation(7)[:c.cout] - 3.0) if c.bias else None            # distinct per channel
    return dict(x=x, w=w, bias=bias)


def _thin_axis(n_in: int, defect=None):
    """per output coordinate o < 2 n_in the two candidate (tap, source) pairs of convT3d_thin_kernel / convT3d_c1_gather_kernel:
    even o: tap 1 from o / 2; odd o: tap 0 from (o + 1) / 2 when that source exists, tap 2 from (o - 1) / 2"""
    o = np.arange(2 * n_in)
    even = o % 2 == 0
    t0, s0 = np.where(even, 1, 0), np.where(even, o // 2, (o + 1) // 2)
    v0 = even | (s0 < n_in)
    t1, s1, v1 = np.full_like(o, 2), (o - 1) // 2, ~even
    if defect == "taps_swapped":
        t0, t1 = np.where(even, 1, 2), np.full_like(o, 0)
    if defect == "clamped":                     # the last odd coordinate takes the last source instead of none
        v0 = np.ones_like(v0)
    if defect == "source_off":
        s0, s1 = s0 + 1, s1 + 1
    s0, s1 = np.clip(s0, 0, n_in - 1), np.clip(s1, 0, n_in - 1)
    return ((t0, s0, v0), (t1, s1, v1))


def _thin_cap_closed_form(c: ThinCase) -> np.ndarray:
    """the cap case: one live input channel, so the output is the ONE-channel fp64 transposed conv of that channel's field"""
    d = thin_operands(c)
    x5 = torch.from_numpy(np.ascontiguousarray(d["x"][..., 5:6])).permute(0, 4, 1, 2, 3)
    y = torch.nn.functional.conv_transpose3d(x5, torch.from_numpy(d["w"][5:6]), torch.from_numpy(d["bias"]), stride=2, padding=1,
                                             output_padding=1)
    return y.permute(0, 2, 3, 4, 1).contiguous().numpy()


def thin_model(c: ThinCase, defect=None, arg=None) -> np.ndarray:
    """(N, 2D, 2H, 2W, C_out) as stored, float64, from the kernels' index arithmetic with at most one defect (the cap case: from
    its closed form, and the one defect it is there for)"""
    d = thin_operands(c)
    if c.kind == "cap":
        out = store(_thin_cap_closed_form(c), c.dt)
        if defect == "one_trip":
            out.reshape(-1, c.cout)[THIN_MAX_BLOCKS * THIN_BLOCK:] = np.nan
        return out
    x, w = d["x"], d["w"].reshape(c.cin, c.cout, 27)
    if defect == "layout_transposed":           # [c][o][t] read as [t][o][c]
        w = d["w"].reshape(27, c.cout, c.cin).transpose(2, 1, 0)
    if defect == "drop_chunk":
        x = x.copy()
        x[..., 8 * arg:8 * arg + 8] = 0
    if defect == "sample0":
        x = np.broadcast_to(x[:1], x.shape)
    wt = np.ascontiguousarray(w.transpose(2, 0, 1))           # (27, C_in, C_out)
    axes = [_thin_axis(c.grid[a], defect if arg == a else None) for a in range(3)]
    out = np.zeros((c.N, *c.out_grid, c.cout))
    for (tz, sz, vz), (ty, sy, vy), (tx, sx, vx) in itertools.product(*axes):
        valid = vz[:, None, None] & vy[None, :, None] & vx[None, None, :]
        if not valid.any():
            continue
        tap = (tz[:, None, None] * 3 + ty[None, :, None]) * 3 + tx[None, None, :]
        out += np.einsum("nzyxc,zyxco->nzyxo", x[:, sz][:, :, sy][:, :, :, sx], wt[tap]) * valid[None, ..., None]
    if d["bias"] is not None:
        out += d["bias"][0] if defect == "bias0" else d["bias"]
    return store(out, c.dt, trunc=defect == "trunc_store")


def thin_reference(c: ThinCase) -> np.ndarray:
    """torch conv_transpose3d in fp64, channels-last"""
    d = thin_operands(c)
    x = torch.from_numpy(d["x"]).permute(0, 4, 1, 2, 3)
    b = torch.from_numpy(d["bias"]) if d["bias"] is not None else None
    y = torch.nn.functional.conv_transpose3d(x, torch.from_numpy(d["w"]), b, stride=2, padding=1, output_padding=1)
    return y.permute(0, 2, 3, 4, 1).contiguous().numpy()


def thin_defects(c: ThinCase):
    if c.kind == "round":
        return [("trunc_store", None)]
    if c.kind == "cap":
        return [("one_trip", None)]
    out = [("drop_chunk", k) for k in range(c.cin // 8)] + [("layout_transposed", None)]
    for a in range(3):
        out += [("taps_swapped", a), ("clamped", a)]
        if c.grid[a] > 1:
            out.append(("source_off", a))
    if c.N > 1:
        out.append(("sample0", None))
    if c.bias and c.cout > 1:
        out.append(("bias0", None))
    return out


@functools.lru_cache(maxsize=4)
def thin_premises(c: ThinCase) -> dict:
    d = thin_operands(c)
    assert _same(store(d["x"], c.dt), d["x"]) and _same(store(d["w"], "f32"), d["w"])
    worst = 8.0 * float(np.abs(d["x"]).reshape(-1, c.cin).max(0) @ np.abs(d["w"]).reshape(c.cin, -1).max(1))
    worst += float(np.abs(d["bias"]).max()) if d["bias"] is not None else 0.0
    R.assert_exact_cap(worst, 1.0, what=c.id)                 # at most 8 taps of C_in integer products each
    y = thin_model(c)
    if c.kind == "cap":                                       # the closed form against a small crop computed in full
        ref = _thin_cap_closed_form(c)
        live = [i for i in range(c.cin) if np.any(d["w"][i] != 0)]
        assert live == [5] and thin_trips(c.outputs) == 2
    else:
        ref = thin_reference(c)
    assert _same(y, store(ref, c.dt)), f"{c.id}: the index model and the fp64 reference differ"
    if c.kind == "round":
        assert (y == np.array([256.0, 260.0, 260.0])).all() and (ref == np.array([257.0, 259.0, 261.0])).all()
    elif c.dt == "bf16":
        assert float(np.abs(ref).max()) <= BF16_INT_CAP and _same(y, ref), f"{c.id}: |reference| over {BF16_INT_CAP} in bf16"
    return dict(y=y, worst=worst)


def thin_discrimination(c: ThinCase) -> dict:
    ref = thin_premises(c)["y"]
    return {(name, arg): changed(thin_model(c, name, arg), ref) for name, arg in thin_defects(c)}


# =====================================================================================================================
# C. RSUNet's bilinear up-sampling: the depthwise transposed conv dwconvT3d_generic_kernel / dwconvT3d_generic_vec_kernel
# (csrc/norm_pool_kernels.hip) and its adjoint dwconv3d_generic_kernel (csrc/rsunet_train_kernels.hip).  Inputs are ternary x 64; the
# bilinear taps are multiples of 1/16, so every term is a multiple of 4, every partial sum is exact and every result is a number of
# both storage types (asserted per case).  The generic geometry has ternary taps that differ per channel.
# =====================================================================================================================
VEC_ELEMS = {"bf16": 8, "f32": 4}          # elems_per_16b_of<T>: the vector kernel runs when C is a multiple of it
DW_SCALE = 64.0
DW_CHANNELS = (1, 4, 6, 8)                 # scalar in both types; vector in fp32 only; scalar in both; vector in both
DW_GRIDS = ((1, 1, 1), (2, 3, 5), (3, 6, 7))
DW_SIGNS = (1.0, -1.0, 1.0, 1.0, -1.0, -1.0, -1.0, 1.0, 1.0, 1.0, 1.0, -1.0, 1.0, 1.0, -1.0, 1.0)
DW_GENERIC = dict(kernel=(3, 5, 2), stride=(3, 2, 1), pad=(0, 2, 1))


def dw_vectorised(C: int, dt: str) -> bool:
    return C % VEC_ELEMS[dt] == 0


def bilinear_geometry(factor):
    """(kernel, stride, pad, plane taps (kd*kh*kw,) float64) of models.architectures.rsunet.BilinearUp3d(C, C, factor)"""
    import sys
    from pathlib import Path
    root = str(Path(__file__).resolve().parents[1])
    if root not in sys.path:
        sys.path.insert(0, root)
    from pytorch_connectomics_amd.models.architectures.rsunet import BilinearUp3d
    m = BilinearUp3d(1, 1, tuple(factor))
    return tuple(m.kernel_size), tuple(m.factor), tuple(m.padding), m.weight.detach().double().reshape(-1).numpy()


@dataclass(frozen=True)
class DwCase:
    dt: str
    geo: str                  # "up122" | "up222" | "generic"
    C: int
    grid: tuple               # input grid of the transposed conv
    N: int

    @property
    def id(self):
        return f"dw-{self.geo}-{self.dt}-c{self.C}-in{'x'.join(map(str, self.grid))}-n{self.N}"


def dw_cases():
    out = []
    for dt in ("bf16", "f32"):
        for geo in ("up122", "up222", "generic"):
            for j, C in enumerate(DW_CHANNELS):
                for k, g in enumerate(DW_GRIDS):
                    if geo == "generic" and g == (1, 1, 1):
                        g = (1, 1, 2)           # its output is empty on one voxel ((1 - 1) 1 - 2 + 2 = 0 along x): the smallest grid
                    out.append(DwCase(dt, geo, C, g, 1 if (j + k) % 2 else 3))
            out.append(DwCase(dt, geo, 6, (2, 3, 5), 3))
            out.append(DwCase(dt, geo, 8, (3, 6, 7), 3))
    return out


@functools.lru_cache(maxsize=None)
def dw_geometry(c: DwCase):
    """(kernel, stride, pad, taps (kd*kh*kw, C) float64, output grid)"""
    if c.geo == "generic":
        k, s, p = DW_GENERIC["kernel"], DW_GENERIC["stride"], DW_GENERIC["pad"]
        taps = _np(R.ternary((k[0] * k[1] * k[2], c.C), 1.0, 77 + c.C, dtype=torch.float32))
    else:
        k, s, p, plane = bilinear_geometry({"up122": (1, 2, 2), "up222": (2, 2, 2)}[c.geo])
        taps = np.repeat(plane[:, None], c.C, axis=1)
    out = tuple((g - 1) * s[a] - 2 * p[a] + k[a] for a, g in enumerate(c.grid))
    return k, s, p, taps, out


@functools.lru_cache(maxsize=4)
def dw_operands(c: DwCase) -> dict:
    seed = zlib.crc32(c.id.encode())
    out = dw_geometry(c)[4]
    x = _np(R.ternary((c.N, *c.grid, c.C), 0.7, seed, dtype=torch.float32))
    dy = _np(R.ternary((c.N, *out, c.C), 0.7, seed + 1, dtype=torch.float32))
    small = lambda a: a if a.size > len(DW_SIGNS) else np.array(DW_SIGNS[:a.size]).reshape(a.shape)
    x, dy = small(x), small(dy)                 # too few values to draw: a fixed sign sequence, no two samples alike
    return dict(x=DW_SCALE * x, dy=DW_SCALE * dy)


def _dwT_axis(n_in, n_out, k, s, p, defect=None):
    """transposed, gather form: for each tap kk the source (o + p - kk) / s of every output coordinate and whether it exists"""
    o = np.arange(n_out)
    for kk in range(k - 1 if defect == "tap_dropped" and k > 1 else k):
        t = o + p - kk
        src = t // s
        valid = (t >= 0) & (src < n_in)
        if defect != "no_remainder_test":
            valid &= t % s == 0
        if defect == "clamped":
            valid = (t >= 0) & (t % s == 0)
        if defect == "source_off":
            src = src + 1
        yield kk, np.clip(src, 0, n_in - 1), valid


def _dw_axis(n_in, n_out, k, s, p, defect=None):
    """plain conv, gather form: tap kk reads o s - p + kk"""
    o = np.arange(n_out)
    for kk in range(k - 1 if defect == "tap_dropped" and k > 1 else k):
        src = o * s - p + kk
        valid = (src >= 0) & (src < n_in)
        if defect == "clamped":
            valid = np.ones_like(valid)
        if defect == "source_off":
            src = src + 1
        yield kk, np.clip(src, 0, n_in - 1), valid


def dw_model(c: DwCase, mode: str, defect=None, arg=None) -> np.ndarray:
    """mode "fwd": the transposed conv of x, (N, out grid, C); mode "bwd": the conv of dy back onto the input grid; as stored"""
    k, s, p, taps, og = dw_geometry(c)
    d = dw_operands(c)
    src_t, n_in, n_out, axis_fn = (d["x"], c.grid, og, _dwT_axis) if mode == "fwd" else (d["dy"], og, c.grid, _dw_axis)
    if defect == "sample0":
        src_t = np.broadcast_to(src_t[:1], src_t.shape)
    w = taps.reshape(*k, c.C)
    if defect == "taps_transposed":             # [kz][ky][kx] read as [kz][kx][ky]
        w = taps.reshape(k[0], k[2], k[1], c.C).transpose(0, 2, 1, 3)
    if defect == "neighbour_channel":
        w = np.roll(w, 1, axis=3)
    axes = [list(axis_fn(n_in[a], n_out[a], k[a], s[a], p[a], defect if arg == a else None)) for a in range(3)]
    out = np.zeros((c.N, *n_out, c.C))
    for (kz, sz, vz), (ky, sy, vy), (kx, sx, vx) in itertools.product(*axes):
        valid = vz[:, None, None] & vy[None, :, None] & vx[None, None, :]
        if valid.any():
            out += src_t[:, sz][:, :, sy][:, :, :, sx] * w[kz, ky, kx] * valid[None, ..., None]
    return store(out, c.dt)


def dw_reference(c: DwCase):
    """torch fp64: conv_transpose3d with groups = C, and the conv3d that is its adjoint -> (y, dx) channels-last"""
    k, s, p, taps, og = dw_geometry(c)
    d = dw_operands(c)
    w = torch.from_numpy(np.ascontiguousarray(taps.T)).reshape(c.C, 1, *k)
    cf = lambda a: torch.from_numpy(a).permute(0, 4, 1, 2, 3)
    y = torch.nn.functional.conv_transpose3d(cf(d["x"]), w, None, stride=s, padding=p, groups=c.C)
    dx = torch.nn.functional.conv3d(cf(d["dy"]), w, None, stride=s, padding=p, groups=c.C)
    last = lambda t: t.permute(0, 2, 3, 4, 1).contiguous().numpy()
    return last(y), last(dx)


def dw_defects(c: DwCase):
    k, s, p, _, og = dw_geometry(c)
    out = []
    for mode in ("fwd", "bwd"):
        for a in range(3):
            n_in, n_out, fn = (c.grid, og, _dwT_axis) if mode == "fwd" else (og, c.grid, _dw_axis)
            listing = lambda defect: [(kk, src[v].tolist(), v.tolist()) for kk, src, v in fn(n_in[a], n_out[a], k[a], s[a], p[a], defect) if v.any()]
            # a defect applies on an axis where it changes which (tap, source) pairs some output coordinate sums
            out += [(mode, name, a) for name in ("tap_dropped", "clamped", "source_off", "no_remainder_test")
                    if (mode == "fwd" or name != "no_remainder_test") and listing(name) != listing(None)]
        if c.N > 1:
            out.append((mode, "sample0", None))
        if c.geo == "generic":                  # the bilinear plane is symmetric and the same for every channel
            out.append((mode, "taps_transposed", None))
            if c.C > 1:
                out.append((mode, "neighbour_channel", None))
    return out


@functools.lru_cache(maxsize=4)
def dw_premises(c: DwCase) -> dict:
    k, s, p, taps, og = dw_geometry(c)
    d = dw_operands(c)
    assert _same(store(d["x"], c.dt), d["x"]) and _same(store(d["dy"], c.dt), d["dy"]) and _same(store(taps, "f32"), taps)
    unit = DW_SCALE * (1.0 if c.geo == "generic" else 1.0 / 16.0)
    assert _same(np.rint(d["x"][..., None, :] * taps / unit) * unit, d["x"][..., None, :] * taps), "a term is no multiple of the unit"
    R.assert_exact_cap(DW_SCALE * float(np.abs(taps).sum(0).max()), unit, what=c.id)
    y64, dx64 = dw_reference(c)
    assert y64.shape[1:4] == og and dx64.shape[1:4] == c.grid, f"{c.id}: the pair's grids do not close"
    y, dx = dw_model(c, "fwd"), dw_model(c, "bwd")
    assert _same(y, y64) and _same(dx, dx64), f"{c.id}: a result is no {c.dt} number, or the index model and the reference differ"
    if c.geo != "generic":
        assert float(np.abs(y64).max()) <= 2 * DW_SCALE and _same(np.rint(y64), y64)        # taps sum to at most 2 per output
    assert float((d["dy"] * y64).sum()) == float((dx64 * d["x"]).sum())                     # the pair is adjoint, in integers
    return dict(y=y, dx=dx)


def dw_discrimination(c: DwCase) -> dict:
    ref = dw_premises(c)
    return {(m, n, a): changed(dw_model(c, m, n, a), ref["y" if m == "fwd" else "dx"]) for m, n, a in dw_defects(c)}

"""Exact-arithmetic cases for the dense 3-D convolutions (CPU only; the one thing taken from the product is the host query
pytc_conv3d_launch_plan, which says which kernel and launch form a shape takes).

Two data sets per case, both free of rounding before the final store, so a kernel must reproduce the fp64 reference BIT FOR BIT:

  dense    x integers in [-2, 2]; pre-activation f(x) = act(a x + b) with a in {1/2, 1, 2}, b in {-1, 0, 1} per (n, c) and act in
           {identity, ReLU, LeakyReLU(1/2)}; weights integers in [-2, 2], bias integers in [-4, 4], residual integers in [-8, 8].
           |a x + b| <= 5 is a multiple of 1/2, the leaky slope makes it a multiple of 1/4 with at most 5 significant bits (bf16 keeps
           8), every product is a multiple of 1/4 of magnitude <= 10, and every partial sum -- in ANY order -- is a multiple of 1/4
           bounded by  5 * 2 * taps * C_in + 12  (34 572 at 27 x 128, 40 012 at 125 x 32): below 2^22, where fp32 holds every multiple of 1/4.  The
           only rounding is the single bf16 store of the result.  b != 0 under an activation makes f(0) != 0: zero padding applied
           to X instead of f(X) changes the border voxels.
  impulse  no pre-activation, bias or residual; x is zero except for isolated ones whose footprints do not overlap (the host test
           proves it with an all-ones kernel), at every volume corner, both voxels either side of every tile seam per axis
           (z 3 | 4, y 7 | 8, x 15 | 16), the volume centre and a lattice of further voxels; the channel of the impulse rotates so that
           every input channel is hit.  Weights are bf16-exact integers in [-127, 127] \\ {0} coded from (o, c, tap): every output is
           exactly one weight or zero, so a wrong (tap, channel, voxel, output channel) mapping shows with nothing rounded away.

References are float64 on the CPU (F.conv3d, F.conv_transpose3d, torch.autograd.grad of the fp64 forward for data gradients), then
ONE round-to-nearest-even to the case's dtype (exact values below 2^22 in quarters are exact in fp32, so the double -> float -> bf16
conversion rounds once).

The case table is a covering set.  Sizes follow the launch rules as read -- MT starts at 4 / 2 / 1 by ceil(C_out / 16) and halves
while  tiles * ceil(MTt / MT) < 256  (phase launch: tiles * 8 * ceil(MTt / MT) < 512); the base grid 5 x 9 x 17 is 2 x 2 x 2 tiles of
4 x 8 x 16 with a one-voxel overhang tile per axis, so N = 32 / 16 reaches 256 workgroups -- and every case states the form and MT it
is filed under; tests/test_host_dense_conv_exact_cases.py checks each against the query, so a retuned threshold cannot move the table
off a form silently."""
from __future__ import annotations

import ctypes as C
import itertools
from dataclasses import dataclass, replace
from functools import lru_cache

import torch
import torch.nn.functional as F

BF16, F32 = torch.bfloat16, torch.float32
TILE = (4, 8, 16)                      # (z, y, x) voxels of a workgroup of the LDS-tiled kernel
STENCIL, TILED, GATHER, THIN = 0, 1, 2, 3
STRIDED = -1                           # conv3d_strided: not a form of the query (its MT depends on C_out only)
PRES = ("none", "affine", "relu", "affine_leaky")
LEAKY = 0.5
OPERAND_COMBOS = tuple(itertools.product(PRES, (False, True), (False, True)))       # (pre, bias, residual): 16
BASE = (5, 9, 17)


@dataclass(frozen=True)
class Case:
    group: str                 # tile | dgrad | phase | stencil | thin | gather | strided
    name: str
    N: int
    dims: tuple                # the grid of the kernel's INPUT tensor (tile / phase forms: the grid the kernel walks)
    cin: int                   # channels of the kernel's input tensor
    cout: int                  # channels it writes
    kernel: tuple = (3, 3, 3)
    dtype: torch.dtype = BF16
    layout: str = "fwd"        # fwd | dgrad | dgrad_padded | convT_phase | conv_dgrad_phase | conv | convT | conv_dgrad | convT_dgrad
    stride: tuple = (1, 1, 1)
    operands: tuple = (("none", False, False),)      # (pre, bias, residual) combinations the dense set runs with
    form: int = TILED
    mt: int = 1                # tiles per workgroup the case is filed under (stencil: channels per thread)
    real: tuple = ()           # dgrad_padded: (cin, cout) that carry data; the rest is alignment padding
    out_odd: bool = False      # conv_dgrad: the strided conv's input grid is 2 d - 1 (odd) instead of 2 d on its stride-2 axes

    @property
    def id(self) -> str:
        return f"{self.group}-{self.name}"

    @property
    def taps(self) -> int:
        return self.kernel[0] * self.kernel[1] * self.kernel[2]

    @property
    def phase(self) -> bool:
        return self.layout in ("convT_phase", "conv_dgrad_phase")

    @property
    def out_dims(self) -> tuple:
        d, k, s = self.dims, self.kernel, self.stride
        if self.layout in ("fwd", "dgrad", "dgrad_padded"):
            return tuple(d)
        if self.phase:
            return tuple(2 * v for v in d)
        if self.layout in ("conv", "convT_dgrad"):
            return tuple((d[i] + 2 - k[i]) // s[i] + 1 for i in range(3))
        if self.layout == "convT":
            return tuple((d[i] - 1) * s[i] - 2 + k[i] + (s[i] - 1) for i in range(3))
        if self.layout == "conv_dgrad":
            return tuple(d[i] if s[i] == 1 else (2 * d[i] - 1 if self.out_odd else 2 * d[i]) for i in range(3))
        raise ValueError(self.layout)

    @property
    def weight_shape(self) -> tuple:
        """shape of the fp32 weight the pack reads, in the layout of the torch module it belongs to"""
        ci, co = (self.real or (self.cin, self.cout))
        if self.layout in ("fwd", "conv"):                       # nn.Conv3d [C_out][C_in]
            return (co, ci) + tuple(self.kernel)
        if self.layout in ("dgrad", "dgrad_padded", "conv_dgrad", "conv_dgrad_phase"):      # the forward nn.Conv3d: ci -> ... reversed
            return (ci, co) + tuple(self.kernel)
        if self.layout in ("convT", "convT_phase"):              # nn.ConvTranspose3d [C_in][C_out]
            return (ci, co) + tuple(self.kernel)
        if self.layout == "convT_dgrad":                         # the forward nn.ConvTranspose3d [C_in_T = cout][C_out_T = cin]
            return (co, ci) + tuple(self.kernel)
        raise ValueError(self.layout)


def sum_bound(c: Case) -> int:
    """bound on every partial sum of the dense set: |f| <= 5, |w| <= 2 over every tap and input channel, + |bias| 4 + |residual| 8"""
    return 5 * 2 * c.taps * c.cin + 12


# ------------------------------------------------------------------------------------------------------------- the case table
def _tile_cases():
    T = []

    def add(name, N, cin, cout, mt, kernel=(3, 3, 3), dims=BASE, form=TILED, group="tile"):
        T.append(Case(group, name, N, dims, cin, cout, kernel=kernel, form=form, mt=mt))

    # MT = 4: full groups, a last group with one live tile (80), a second pass with 8 live channels (72)
    add("mt4-c16-o64", 32, 16, 64, 4)
    add("mt4-c32-o128", 16, 32, 128, 4)
    add("mt4-c8-o80", 16, 8, 80, 4)
    add("mt4-c8-o72", 16, 8, 72, 4)
    # MT = 2: cw_live = 24, partial second groups, the case that falls from 4 to 2
    add("mt2-c16-o32", 32, 16, 32, 2)
    add("mt2-c8-o24", 32, 8, 24, 2)
    add("mt2-c8-o48", 16, 8, 48, 2)
    add("mt2-c16-o40", 16, 16, 40, 2)
    add("mt2-c8-o64-from4", 16, 8, 64, 2)
    # MT = 1
    add("mt1-c8-o8", 2, 8, 8, 1)
    add("mt1-c16-o16", 16, 16, 16, 1)
    add("mt1-c8-o64-n1", 1, 8, 64, 1)
    # C_out % 8 != 0: the per-lane epilogue, at each MT the rule gives
    add("odd-o3-mt1", 8, 8, 3, 1)
    add("odd-o20-mt2", 32, 8, 20, 2)
    add("odd-o20-mt1", 2, 16, 20, 1)
    add("odd-o36-mt2", 16, 8, 36, 2)
    add("odd-o36-mt1", 2, 8, 36, 1)
    # C_in: one chunk with a zero-padded last group (8, 16, 24), 27 full groups (32), KC = 8 x 5, 16 x 3, 32 x 2, 32 x 4
    add("cin24-mt2", 32, 24, 32, 2)
    add("cin32-mt1", 32, 32, 16, 1)
    add("cin40-mt4", 32, 40, 64, 4)
    add("cin48-mt2", 32, 48, 32, 2)
    add("cin64-mt4", 32, 64, 64, 4)
    add("cin128-mt4", 16, 128, 128, 4)
    # kernels; (1, 1, 1) at C_in = 8 is ONE group, fewer than the weight ring is deep; 5^3 is tiled at C_in = 8 / 16 only
    add("k133-mt4", 32, 16, 64, 4, kernel=(1, 3, 3))
    add("k311-mt2", 32, 32, 32, 2, kernel=(3, 1, 1))
    add("k111-g1-mt1", 8, 8, 16, 1, kernel=(1, 1, 1))
    add("k111-g1-mt4", 32, 8, 64, 4, kernel=(1, 1, 1))
    add("k555-c8-mt1", 8, 8, 16, 1, kernel=(5, 5, 5))
    add("k555-c16-mt2", 32, 16, 32, 2, kernel=(5, 5, 5))
    add("k555-c32-gather", 32, 32, 16, 1, kernel=(5, 5, 5), form=GATHER, group="gather")
    # geometry: one voxel, planes with no wave and rows shorter than a tile, exactly one tile, a third x tile of one voxel
    add("g1x1x1-mt1", 8, 8, 16, 1, dims=(1, 1, 1))
    add("g2x3x5-mt1", 8, 8, 8, 1, dims=(2, 3, 5))
    add("g2x3x5-mt2", 256, 8, 32, 2, dims=(2, 3, 5))
    add("g4x8x16-mt1", 16, 16, 16, 1, dims=(4, 8, 16))
    add("g3x8x33-mt2", 43, 16, 48, 2, dims=(3, 8, 33))
    add("g3x8x33-mt4", 43, 8, 128, 4, dims=(3, 8, 33))
    # every (pre, bias, residual) combination at every MT: dealt round-robin over the tiled cases of the MT class
    out = []
    for mt in (4, 2, 1):
        cls = [c for c in T if c.form == TILED and c.mt == mt]
        per = -(-len(OPERAND_COMBOS) // len(cls))
        for i, c in enumerate(cls):
            out.append(replace(c, operands=tuple(OPERAND_COMBOS[(i * per + j) % len(OPERAND_COMBOS)] for j in range(per))))
    out += [replace(c, operands=(("affine_leaky", True, True),)) for c in T if c.form != TILED]
    return out


def _dgrad_cases():
    return [
        # the 'dgrad' image (taps mirrored, channels swapped) through the tiled kernel: forward Conv3d(cout -> cin)
        Case("dgrad", "c16-o8-mt1", 4, BASE, 16, 8, layout="dgrad", mt=1, operands=(("none", False, False), ("none", False, True))),
        Case("dgrad", "c24-o64-mt4", 32, BASE, 24, 64, layout="dgrad", mt=4, operands=(("none", False, False),)),
        Case("dgrad", "k133-c48-o80-mt4", 16, BASE, 48, 80, kernel=(1, 3, 3), layout="dgrad", mt=4, operands=(("none", False, True),)),
        # RSUNet's stock width 18 travels as 24 channels: the padded image must ignore what the padding channels of x hold
        Case("dgrad", "padded18-mt2", 32, BASE, 24, 24, layout="dgrad_padded", mt=2, real=(18, 18), operands=(("none", False, False),)),
    ]


def _phase_cases():
    P = []

    def add(name, layout, N, dims, cin, cout, mt, ops):
        P.append(Case("phase", name, N, dims, cin, cout, layout=layout, mt=mt, operands=ops))

    nb, b, r, br = ("none", False, False), ("none", True, False), ("none", False, True), ("none", True, True)
    pre = ("affine_leaky", True, True)
    add("T-c8-o64-mt4", "convT_phase", 8, BASE, 8, 64, 4, (b, r))
    add("T-c32-o80-mt4", "convT_phase", 8, BASE, 32, 80, 4, (br,))
    add("T-c48-o32-mt2", "convT_phase", 8, BASE, 48, 32, 2, (nb, pre))
    add("T-c64-o20-mt2", "convT_phase", 8, BASE, 64, 20, 2, (br,))
    add("T-c8-o8-mt1", "convT_phase", 8, BASE, 8, 8, 1, (b,))
    add("T-c8-o64-mt1-n1", "convT_phase", 1, BASE, 8, 64, 1, (br, nb))
    add("T-c8-o20-mt1-small", "convT_phase", 8, (2, 3, 5), 8, 20, 1, (r,))
    add("T-c8-o64-mt4-small", "convT_phase", 64, (2, 3, 5), 8, 64, 4, (br,))
    add("D-c64-o64-mt4", "conv_dgrad_phase", 8, BASE, 64, 64, 4, (nb,))
    add("D-c8-o80-mt4", "conv_dgrad_phase", 8, BASE, 8, 80, 4, (r,))
    add("D-c32-o32-mt2", "conv_dgrad_phase", 8, BASE, 32, 32, 2, (nb,))
    add("D-c48-o8-mt1", "conv_dgrad_phase", 8, BASE, 48, 8, 1, (nb,))
    add("D-c32-o20-mt2-small", "conv_dgrad_phase", 64, (2, 3, 5), 32, 20, 2, (nb,))
    return P


def _other_cases():
    O = []
    full = (("none", True, False),)
    # one-input-channel stencil (no pre-activation, no residual: it refuses them): stride 1 through conv3d (the query names it), stride 2
    # on the odd base grid through conv3d_strided
    for co, st, dt, oct_ in ((1, 1, BF16, 1), (3, 2, F32, 4), (8, 1, F32, 8), (20, 2, BF16, 8), (32, 1, BF16, 32), (36, 2, F32, 32),
                             (40, 1, F32, 32), (64, 2, BF16, 32), (3, 1, BF16, 4)):
        O.append(Case("stencil", f"s{st}-o{co}-{'bf16' if dt == BF16 else 'f32'}", 2, BASE, 1, co, dtype=dt,
                      layout="fwd" if st == 1 else "conv", stride=(st, st, st), form=STENCIL if st == 1 else STRIDED,
                      mt=oct_ if st == 1 else 0, operands=full if co % 2 == 0 else (("none", False, False),)))
    # thin-input kernel
    O.append(Case("thin", "c2-o20-bf16", 2, BASE, 2, 20, form=THIN, mt=1, operands=(("affine_leaky", True, True),)))
    O.append(Case("thin", "c3-o8-f32", 2, BASE, 3, 8, dtype=F32, form=THIN, mt=1, operands=(("relu", True, False),)))
    O.append(Case("thin", "c4-o36-bf16", 2, BASE, 4, 36, form=THIN, mt=1, operands=(("affine", False, True),)))
    # MFMA gather kernel: fp32, bf16 with C_in % 8 != 0, and the one-channel conv with a pre-activation (the stencil refuses it)
    O.append(Case("gather", "f32-c8-o8", 2, BASE, 8, 8, dtype=F32, form=GATHER, mt=1, operands=(("affine_leaky", True, True),)))
    O.append(Case("gather", "f32-c16-o36", 2, BASE, 16, 36, dtype=F32, form=GATHER, mt=2, operands=(("relu", False, True),)))
    O.append(Case("gather", "f32-c20-o80", 2, BASE, 20, 80, dtype=F32, form=GATHER, mt=4, operands=(("affine", True, False),)))
    O.append(Case("gather", "bf16-c6-o16", 2, BASE, 6, 16, form=GATHER, mt=1, operands=(("affine_leaky", True, True),)))
    O.append(Case("gather", "bf16-c18-o36", 2, BASE, 18, 36, form=GATHER, mt=2, operands=(("relu", True, True),)))
    O.append(Case("gather", "bf16-c20-o64", 2, BASE, 20, 64, form=GATHER, mt=4, operands=(("affine", False, False),)))
    # (the one-channel conv with a pre-activation, which the stencil refuses, is a thin-input launch by the rule C_in <= 4)
    O.append(Case("thin", "c1-o16-bf16-ab", 2, BASE, 1, 16, form=THIN, mt=1, operands=(("affine_leaky", True, False),)))
    # conv3d_strided in its four layouts
    S = dict(form=STRIDED, mt=0)
    O.append(Case("strided", "conv-s222-c8-o24", 2, (5, 9, 17), 8, 24, layout="conv", stride=(2, 2, 2), operands=(("affine_leaky", True, True),), **S))
    O.append(Case("strided", "conv-s122-c16-o64", 2, (5, 9, 17), 16, 64, layout="conv", stride=(1, 2, 2), operands=(("relu", True, False),), **S))
    O.append(Case("strided", "convT-s222-c16-o8", 4, (3, 5, 9), 16, 8, layout="convT", stride=(2, 2, 2), operands=(("none", True, True),), **S))
    O.append(Case("strided", "convT-s122-c8-o64", 2, (3, 5, 9), 8, 64, layout="convT", stride=(1, 2, 2), operands=(("affine", True, False),), **S))
    O.append(Case("strided", "conv_dgrad-s222-c24-o8-odd", 6, (3, 5, 9), 24, 8, layout="conv_dgrad", stride=(2, 2, 2), out_odd=True,
                  operands=(("none", False, False),), **S))
    O.append(Case("strided", "conv_dgrad-s122-c8-o24", 2, (3, 5, 9), 8, 24, layout="conv_dgrad", stride=(1, 2, 2),
                  operands=(("none", False, True),), **S))
    O.append(Case("strided", "convT_dgrad-s222-c8-o64", 2, (6, 10, 18), 8, 64, layout="convT_dgrad", stride=(2, 2, 2),
                  operands=(("none", False, False),), **S))
    O.append(Case("strided", "convT_dgrad-s122-c64-o24-f32", 6, (3, 10, 18), 64, 24, dtype=F32, layout="convT_dgrad", stride=(1, 2, 2),
                  operands=(("none", False, True),), **S))
    return O


@lru_cache(maxsize=None)
def all_cases() -> tuple:
    cs = tuple(_tile_cases() + _dgrad_cases() + _phase_cases() + _other_cases())
    assert len({c.id for c in cs}) == len(cs)
    return cs


def cases(*groups) -> list:
    return [c for c in all_cases() if c.group in groups]


# ------------------------------------------------------------------------------------------------------------- the query
def launch_plan(c: Case, pre: str = "none", res: bool = False):
    """(form, MT, KC, chunks, G, workgroups) from pytc_conv3d_launch_plan for the stride-1 and phase cases, None for conv3d_strided"""
    if c.form == STRIDED:
        return None
    from pytorch_connectomics_amd import _native as nat
    out = (C.c_int64 * 6)()
    nat.check(nat.lib().pytc_conv3d_launch_plan(c.N, *c.dims, c.cin, c.cout, *c.kernel, nat.BF16 if c.dtype == BF16 else nat.F32,
                                                int(pre != "none"), int(res), int(c.phase), out), "conv3d_launch_plan")
    return tuple(int(v) for v in out)


# ------------------------------------------------------------------------------------------------------------- data
def _gen(c: Case, salt: int) -> torch.Generator:
    g = torch.Generator()
    g.manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(c.id)) * 16 + salt)
    return g


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def dense_data(c: Case, combo) -> dict:
    """fp64 operands in torch's layouts: x (N, cin, *dims), w (weight_shape), ab (N, 2, cin) | None, bias (cout) | None,
    res (N, cout, *out_dims) | None, act"""
    pre, has_bias, has_res = combo
    g = _gen(c, 1 + OPERAND_COMBOS.index(tuple(combo)))
    d = {"x": _ints(g, (c.N, c.cin) + tuple(c.dims), -2, 2), "w": _ints(g, c.weight_shape, -2, 2), "ab": None, "bias": None, "res": None,
         "act": {"none": "none", "affine": "none", "relu": "relu", "affine_leaky": "leaky"}[pre]}
    if c.real:                                    # alignment-padding channels of x hold values the image has to ignore
        d["x"][:, c.real[0]:] = _ints(g, (c.N, c.cin - c.real[0]) + tuple(c.dims), 1, 2)
    if pre.startswith("affine"):
        a = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (c.N, c.cin), generator=g)]
        d["ab"] = torch.stack([a, _ints(g, (c.N, c.cin), -1, 1)], 1)
    if has_bias:
        d["bias"] = _ints(g, (c.cout,), -4, 4)
    if has_res:
        d["res"] = _ints(g, (c.N, c.cout) + c.out_dims, -8, 8)
    return d


def _axis_coords(n: int, tile: int) -> list:
    """first and last voxel, and both voxels either side of every tile seam"""
    s = {0, n - 1}
    for seam in range(tile, n, tile):
        s |= {seam - 1, seam}
    return sorted(s)


def impulse_positions(c: Case) -> list:
    """[(n, z, y, x, channel)], footprints (kernel-sized boxes, whatever the stride) pairwise disjoint within a sample.  REQUIRED, or an
    AssertionError: the eight corners, and per axis every coordinate of _axis_coords (borders and both sides of every seam) at some
    voxel.  Then, where they still fit: the centre, every combination of those coordinates over the three axes (seams crossed in two
    and three axes at once), and a lattice of further voxels until every input channel has an impulse.  channel = running index mod
    the input channels that carry data."""
    D, H, W = c.dims
    k = c.kernel
    cin = c.real[0] if c.real else c.cin
    ax = [_axis_coords(n, t) for n, t in zip(c.dims, TILE)]
    placed, per_sample, seen = [], [[] for _ in range(c.N)], set()

    def place(p) -> bool:
        if p in seen:
            return True
        for t in range(c.N):
            m = (len(placed) + t) % c.N                        # spread over the batch
            if all(any(abs(p[a] - q[a]) >= k[a] for a in range(3)) for q in per_sample[m]):
                per_sample[m].append(p)
                placed.append((m,) + p + (len(placed) % cin,))
                seen.add(p)
                return True
        return False

    for p in itertools.product((0, D - 1), (0, H - 1), (0, W - 1)):
        assert place(p), f"{c.id}: corner {p} fits no sample (N = {c.N})"
    place((D // 2, H // 2, W // 2))
    for a in range(3):
        o1, o2 = [b for b in range(3) if b != a]
        for v in ax[a]:
            # the voxel's other two coordinates: from the centre outwards until it fits
            cand = sorted(itertools.product(range(c.dims[o1]), range(c.dims[o2])),
                          key=lambda uv: (abs(uv[0] - c.dims[o1] // 2) + abs(uv[1] - c.dims[o2] // 2), uv))
            for u, w_ in cand:
                p = [0, 0, 0]
                p[a], p[o1], p[o2] = v, u, w_
                if tuple(p) not in seen and place(tuple(p)):
                    break
            else:                                              # (a corner may hold the coordinate already)
                assert any(q[a] == v for q in seen), f"{c.id}: no room for an impulse at axis {a} coordinate {v} (N = {c.N})"
    for p in itertools.product(*ax):
        place(p)
    lattice = list(itertools.product(range(1 if D > 1 else 0, D, k[0]), range(1 if H > 1 else 0, H, k[1]),
                                     range(1 if W > 1 else 0, W, k[2])))
    for _ in range(c.N):
        for p in lattice:
            if len(placed) >= cin:
                return placed
            seen.discard(p)
            place(p)
            seen.add(p)
    return placed


def impulse_weight(c: Case) -> torch.Tensor:
    """bf16-exact integers in [-127, 127] without 0, coded from the flat (dim 0, dim 1, tap) index of the weight tensor"""
    shape = c.weight_shape
    n = 1
    for v in shape:
        n *= v
    i = torch.arange(n, dtype=torch.int64)
    v = (i * 37 + (i // shape[1] // c.taps) * 11 + 5) % 254         # 0 .. 253
    return (v - 127 + (v >= 127).long()).double().view(shape)     # -127 .. -1, 1 .. 127


def impulse_data(c: Case) -> dict:
    x = torch.zeros((c.N, c.cin) + tuple(c.dims), dtype=torch.float64)
    for n, z, y, xx, ch in impulse_positions(c):
        x[n, ch, z, y, xx] = 1.0
    return {"x": x, "w": impulse_weight(c), "ab": None, "bias": None, "res": None, "act": "none"}


# ------------------------------------------------------------------------------------------------------------- references
def pre_activation(x: torch.Tensor, ab, act: str) -> torch.Tensor:
    if ab is not None:
        x = x * ab[:, 0][:, :, None, None, None] + ab[:, 1][:, :, None, None, None]
    if act == "relu":
        x = x.clamp_min(0)
    elif act == "leaky":
        x = torch.where(x > 0, x, x * LEAKY)
    return x


def linear_part(c: Case, fx: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """the convolution of the case in the dtype of its operands: (N, cout, *out_dims)"""
    k, s = c.kernel, c.stride
    same = tuple(v // 2 for v in k)
    if c.layout == "fwd":
        return F.conv3d(fx, w, padding=same)
    if c.layout in ("dgrad", "dgrad_padded"):
        ci, co = c.real or (c.cin, c.cout)
        z = torch.zeros((c.N, co) + tuple(c.dims), dtype=fx.dtype, requires_grad=True)
        (g,) = torch.autograd.grad(F.conv3d(z, w, padding=same), z, grad_outputs=fx[:, :ci].contiguous(), create_graph=w.requires_grad)
        return F.pad(g, (0, 0, 0, 0, 0, 0, 0, c.cout - co)) if c.real else g
    if c.layout == "convT_phase":
        return F.conv_transpose3d(fx, w, stride=2, padding=1, output_padding=1)
    if c.layout in ("conv_dgrad_phase", "conv_dgrad"):
        st = 2 if c.phase else s
        z = torch.zeros((c.N, c.cout) + c.out_dims, dtype=fx.dtype, requires_grad=True)
        y = F.conv3d(z, w, stride=st, padding=1)
        assert tuple(y.shape[2:]) == tuple(c.dims), (c.id, tuple(y.shape), c.dims)
        (g,) = torch.autograd.grad(y, z, grad_outputs=fx, create_graph=w.requires_grad)
        return g
    if c.layout == "conv":
        return F.conv3d(fx, w, stride=s, padding=1)
    if c.layout == "convT":
        return F.conv_transpose3d(fx, w, stride=s, padding=1, output_padding=tuple(v - 1 for v in s))
    if c.layout == "convT_dgrad":
        z = torch.zeros((c.N, c.cout) + c.out_dims, dtype=fx.dtype, requires_grad=True)
        y = F.conv_transpose3d(z, w, stride=s, padding=1, output_padding=tuple(v - 1 for v in s))
        assert tuple(y.shape[2:]) == tuple(c.dims), (c.id, tuple(y.shape), c.dims)
        (g,) = torch.autograd.grad(y, z, grad_outputs=fx, create_graph=w.requires_grad)
        return g
    raise ValueError(c.layout)


def reference64(c: Case, d: dict) -> torch.Tensor:
    """float64 (N, cout, *out_dims): conv(f(x)) + bias + residual, before the one rounding of the store"""
    y = linear_part(c, pre_activation(d["x"], d["ab"], d["act"]), d["w"])
    if d["bias"] is not None:
        y = y + d["bias"][None, :, None, None, None]
    if d["res"] is not None:
        y = y + d["res"]
    return y.detach()


def reference(c: Case, d: dict) -> torch.Tensor:
    """the expected output tensor: reference64 rounded once (to nearest even) to the case's dtype"""
    return reference64(c, d).to(c.dtype)


def channels_last(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 2, 3, 4, 1).contiguous()


def channels_first(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 4, 1, 2, 3).contiguous()

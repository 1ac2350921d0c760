"""CPU checks of tests/stencil_exact_cases.py.  Three things are proven here, without a GPU:

  1. the exactness premises hold for every case (f16 in-plane sums, fp32 accumulators, both statistics bounds, f16-exact stem
     products, outputs bf16 cannot represent -- ties and non-ties -- where the case asks for them), and every case is filed under the
     kernel variant, slot count, z-chunking and raggedness that the mirrors AND the library's own host queries give it;
  2. a correct kernel passes: an fp32 restatement of each form -- taps in (kz, ky, kx) order, the packed-f16 nine-tap partial sums of
     the dwconv_march_h16 form, the bf16 hi (+ lo) weight halves of the matrix-core form, the cell arithmetic of the transposed forms,
     the border constants of the two stem forms, ONE rounding, statistics of the STORED values summed per slot in fp32 -- equals the
     fp64 reference bit for bit, output, per-slot partials and totals;
  3. seeded defects fail: each of the eleven defects below (nineteen runs), put into that restatement, changes the output or the statistics of the case
     it is run on, so the exact comparison of tests/test_gpu_stencil_exact.py sees a kernel that has it."""
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import stencil_exact_cases as X  # noqa: E402

ALL = X.all_cases()
IDS = [c.id for c in ALL]
BY_ID = {c.id: c for c in ALL}


# ------------------------------------------------------------------------------------------------------------- the restatement
def _store(acc: torch.Tensor, dtype, mode: str = "rne") -> torch.Tensor:
    if dtype == X.F32 or mode == "rne":
        return acc.to(dtype)
    bits = acc.contiguous().view(torch.int32)
    if mode == "half_up":                       # round half away from zero in magnitude: + 0x8000, truncate
        bits = bits + 0x8000
    return (bits & -65536).view(torch.float32).to(dtype)


def _conv_acc(c, d, defect):
    """fp32 accumulator (N, Do, Ho, Wo, C) of the plain / strided conv forms, taps in (kz, ky, kx) order"""
    K, P, s = c.K, c.K // 2, c.stride
    Do, Ho, Wo = c.out_dims
    f = X.form(c)
    x, w = d["x"].float(), d["w"].float()
    if defect == "flip_taps":
        w = w.flip(0)
    if defect == "lost_cg_offset":              # the second channel group reads the first group's taps
        w = w.clone()
        w[:, 32:] = w[:, :c.C - 32]
    h16 = f == "march" and c.dtype == X.BF16 and c.entry == "fwd" and c.knob["dwconv_march_h16"] != 0
    lo = f == "mfma" and bool((c.knob["dwconv_mfma_variant"] & 1) or not X.march_ok(*c.dims, c.C, c.K, c.stride, c.dtype, False))
    w_hi = w.to(X.BF16).float() if f == "mfma" else w
    w_lo = (w - w_hi).to(X.BF16).float()
    acc = d["bias"].float().expand(c.N, Do, Ho, Wo, c.C).clone()
    xp = F.pad(x, (0, 0, P, P, P, P, P, P))
    for kz in range(K):
        part = None
        for ky in range(K):
            for kx in range(K):
                t = (kz * K + ky) * K + kx
                xs = xp[:, kz:kz + s * (Do - 1) + 1:s, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s]
                if (defect == "drop_face_tap" and (kz, ky, kx) == (1, 1, 0)) or (defect == "s2_even_tap_padded" and kx == 2):
                    xs = xs.clone()
                    xs[:, :, :, Wo - 1] = 0     # a tap INSIDE the volume lost at the x = max face
                if h16:
                    pr = xs.half() * w[t].half()
                    part = pr if part is None else part + pr
                else:
                    acc = acc + xs * w_hi[t]
                    if lo:
                        acc = acc + xs * w_lo[t]
        if h16:
            acc = acc + part.float()
    return acc


def _convT_acc(c, d, defect):
    """fp32 accumulator on the (2D, 2H, 2W) grid: position p holds the transposed conv's output p - 1 = 2 i - P + k; front planes not yet zeroed"""
    K, P = c.K, c.K // 2
    x, w = d["x"].float(), d["w"].float()
    if defect == "flip_taps":
        w = w.flip(0)
    acc = d["bias"].float().expand((c.N,) + c.out_dims + (c.C,)).clone()

    def rng(k, n):                               # input indices i with 1 <= 2 i + k - P + 1 <= 2 n - 1
        off = k - P + 1
        i0 = max(0, -((off - 1) // 2))
        i1 = min(n - 1, (2 * n - 1 - off) // 2)
        return i0, i1, off

    for kz in range(K):
        z0, z1, oz = rng(kz, c.dims[0])
        for ky in range(K):
            y0, y1, oy = rng(ky, c.dims[1])
            for kx in range(K):
                x0, x1, ox = rng(kx, c.dims[2])
                if z1 < z0 or y1 < y0 or x1 < x0:
                    continue
                acc[:, 2 * z0 + oz:2 * z1 + oz + 1:2, 2 * y0 + oy:2 * y1 + oy + 1:2, 2 * x0 + ox:2 * x1 + ox + 1:2] += \
                    x[:, z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] * w[(kz * K + ky) * K + kx]
    return acc


def _bwd_acc(c, d):
    """fp32 accumulator of the data gradient: dx[i] = sum_k dy[(i + P - k) / s] w[k], i.e. i = s o - P + k"""
    K, P, s = c.K, c.K // 2, c.stride
    dy, w = d["x"].float(), d["w"].float()
    acc = torch.zeros((c.N,) + tuple(c.xdims) + (c.C,), dtype=torch.float32)

    def rng(k, n_o, n_i):
        off = k - P
        o0 = max(0, -(off // s))
        o1 = min(n_o - 1, (n_i - 1 - off) // s)
        return o0, o1, off

    for kz in range(K):
        z0, z1, oz = rng(kz, c.dims[0], c.xdims[0])
        for ky in range(K):
            y0, y1, oy = rng(ky, c.dims[1], c.xdims[1])
            for kx in range(K):
                x0, x1, ox = rng(kx, c.dims[2], c.xdims[2])
                if z1 < z0 or y1 < y0 or x1 < x0:
                    continue
                acc[:, s * z0 + oz:s * z1 + oz + 1:s, s * y0 + oy:s * y1 + oy + 1:s, s * x0 + ox:s * x1 + ox + 1:s] += \
                    dy[:, z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] * w[(kz * K + ky) * K + kx]
    return acc


def _stem_acc(c, d, defect):
    """VALU form: cst + sum wx x - sum over taps OUTSIDE the volume of wb, cst = bias + sum wb.  Matrix-core form: border blocks
    (bias alone) + sum f16(wx) f16(x) + sum over taps INSIDE of f16(wb); interior blocks cst + sum f16(wx) f16(x)"""
    D, H, W = c.dims
    x = d["x"].float()
    wx = (d["w"] * d["stem_w"]).float()
    wb = (d["w"] * d["stem_b"]).float()
    cst = wb.sum(0) + d["bias"].float()
    mf = X.form(c) == "stem_mfma"
    if mf:
        wx, wb = wx.half().float(), wb.half().float()
        x = x.half().float()
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
    ins = F.pad(torch.ones((1, D, H, W)), (1, 1, 1, 1, 1, 1))
    border = torch.zeros((D, H, W), dtype=torch.bool)
    if mf:                                       # 8 x 8 x 16 blocks that touch a face of the volume
        z, y, xx = X._grid((D, H, W))
        border = ((z // 8 == 0) | (z // 8 == D // 8 - 1) | (y // 8 == 0) | (y // 8 == H // 8 - 1) | (xx // 16 == 0) | (xx // 16 == W // 16 - 1))
    acc = cst.expand(c.N, D, H, W, 32).clone()
    if mf:
        acc = torch.where(border[None, :, :, :, None], (cst - wb.sum(0)).expand_as(acc), acc)
    for t in range(27):
        kz, ky, kx = t // 9, t // 3 % 3, t % 3
        xs = xp[:, kz:kz + D, ky:ky + H, kx:kx + W]
        it = ins[:, kz:kz + D, ky:ky + H, kx:kx + W]
        acc = acc + xs[..., None] * wx[t]
        if defect == "stem_bias_outside":       # the stem bias counted for taps that lie outside the volume
            if mf:
                acc = acc + border[None, :, :, :, None] * wb[t]
            continue
        if mf:
            acc = acc + (it * border)[..., None] * wb[t]
        else:
            acc = acc - (1 - it)[..., None] * wb[t]
    return acc


def restate(c, d, defect=None):
    """-> (stored tensor in the case's dtype, fp32 per-slot statistics (N, slots, 2, C) | None) as a kernel of the case's form computes them"""
    mode = {"truncate": "trunc", "half_up": "half_up"}.get(defect, "rne")
    if c.entry == "stem":
        acc = _stem_acc(c, d, defect)
    elif c.entry in ("bwd", "bwd_add"):
        acc = _bwd_acc(c, d)
    elif c.transposed:
        acc = _convT_acc(c, d, defect)
    else:
        acc = _conv_acc(c, d, defect)
    src = acc                                    # what the statistics are taken from
    if c.transposed:
        front = acc.clone()
        acc[:, 0] = 0
        acc[:, :, 0] = 0
        acc[:, :, :, 0] = 0
        src = front if defect == "count_front_plane" else acc
    if d["res"] is not None:
        res = d["res"].float()
        acc = (_store(acc, c.dtype).float() + res) if defect == "two_roundings" else acc + res
    stored = _store(acc, c.dtype, mode)
    if not c.has_stats:
        return stored, None
    sv = src if defect == "stats_unrounded" else _store(src, c.dtype, mode).float()
    if defect == "drop_ragged_stat_voxel":      # the last column of the ragged tile misses the statistics
        sv = sv.clone()
        sv[:, -1, -1, -1] = 0
    sm = X.slot_map(c).reshape(-1)
    st = torch.zeros((c.N, X.mirror_slots(c), 2, c.C), dtype=torch.float32)
    flat = sv.reshape(c.N, -1, c.C)
    st[:, :, 0].index_add_(1, sm, flat)
    st[:, :, 1].index_add_(1, sm, flat * flat)
    return stored, st


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _agrees(c, d, stored, st):
    """(output equal, statistics equal) against the fp64 reference"""
    ok_y = torch.equal(_bits(stored), _bits(d["want"]))
    ok_s = True
    if st is not None:
        ok_s = torch.equal(st.double(), X.slot_stats(c, d["want"])) and torch.equal(st.double().sum(1), X.stats_of(d["want"]))
    return ok_y, ok_s


# ------------------------------------------------------------------------------------------------------------- 1. premises and filing
def test_table_covers_every_form_of_the_issue():
    forms = {X.form(c) for c in ALL}
    assert forms == {"direct", "gather", "xblock", "march", "mfma", "s2", "cell", "generic", "tile", "stem_valu", "stem_mfma", "bwd_vec", "bwd_scalar"}
    assert {c.variant for c in ALL if c.variant >= 0} == set(range(9))
    by = lambda g: [c for c in ALL if c.group == g]                                   # noqa: E731
    assert {c.K for c in by("direct")} == {1, 5, 7} and {(c.K, c.C) for c in by("direct") if c.K > 1} == {(7, 48), (5, 136)}
    assert {(c.C, c.dtype) for c in by("gather")} >= {(4, X.F32), (12, X.F32), (32, X.F32), (5, X.BF16), (6, X.BF16), (12, X.BF16)}
    assert {X.geometry(c)["vec"] for c in by("gather") if c.dtype == X.BF16} >= {1, 2, 4} and {c.K for c in by("gather")} == {3, 5, 7}
    s2g = [c for c in by("gather") if c.stride == 2]
    assert any(all(v % 2 for v in c.dims) for c in s2g) and any(not any(v % 2 for v in c.dims) for c in s2g)
    assert {c.C for c in by("xblock")} == {8, 24, 32, 40} and {c.K for c in by("xblock")} == {3, 5, 7}
    assert {c.dims[2] for c in by("xblock")} >= {4, 5, 6, 7, 9} and {X.geometry(c)["iters"] for c in by("xblock")} == {1, 2}
    march = {(c.dims, c.C) for c in by("march")}
    assert march == {((8, 16, 16), 32), ((9, 17, 19), 32), ((8, 16, 16), 64), ((10, 16, 16), 32), ((11, 17, 16), 32), ((29, 64, 64), 32)}
    assert {(c.dtype, c.knob["dwconv_march_h16"]) for c in by("march")} == {(X.BF16, 1), (X.BF16, 0), (X.F32, 1)}
    assert {X.geometry(c)["min_planes"] for c in by("march") if c.multi_chunk} == {5, 14}
    assert {(c.dims, c.C) for c in by("mfma") if c.name.startswith("v")} >= march
    assert {c.knob["dwconv_mfma_variant"] for c in by("mfma")} == {0, 1, 2, 3} and {c.C for c in by("mfma")} == {32, 64, 96}
    assert {c.dims for c in by("mfma") if "small" in c.name} >= {(8, 8, 9), (10, 15, 8), (14, 14, 14)} and all(c.stats_only for c in by("mfma"))
    assert {(c.dims, c.C) for c in by("s2")} == {(dm, cc) for cc in (32, 64) for dm in ((1, 1, 1), (7, 5, 6), (9, 20, 31), (27, 9, 17), (29, 9, 17), (28, 16, 32))}
    assert {c.C for c in by("cell")} >= {8, 32, 64} and {(c.K, c.C) for c in by("generic")} >= {(5, 8), (7, 12), (3, 608)}
    assert {(c.dims, c.C) for c in by("tile")} == {(dm, cc) for cc in (64, 128) for dm in ((1, 1, 1), (2, 8, 8), (3, 9, 9), (5, 9, 11), (3, 4, 7))}
    assert all(c.stats_only for c in by("tile"))
    stem = {c.dims: X.geometry(c) for c in by("stem")}
    assert {dm for dm, g in stem.items() if g["form"] == "stem_valu"} == {(5, 6, 8), (9, 7, 12), (8, 9, 16)} and stem[(8, 9, 16)]["slots"] == 2
    assert {dm: g["zr"] for dm, g in stem.items() if g["form"] == "stem_mfma"} == {(8, 8, 16): 8, (16, 24, 32): 8, (128, 64, 64): 16, (136, 64, 64): 16,
                                                                                  (256, 64, 64): 32}
    # both z-ranges need 256 workgroups per sample: (128, 64, 64) / (256, 64, 64) are the smallest volumes that reach them with FULL
    # last blocks (8 / 8 z-ranges of 16 / 32 planes; 120 and 232 planes reach them too, with a shorter last range like (136, 64, 64))
    assert X.sd_geom(112, 64, 64)["zr"] == 8 and X.sd_geom(224, 64, 64)["zr"] == 16 and X.sd_geom(128, 64, 48)["zr"] == 8
    assert X.sd_geom(120, 64, 64)["zr"] == 16 and X.sd_geom(232, 64, 64)["zr"] == 32
    bwd = by("bwd")
    assert {(X.form(c), c.C, c.dtype) for c in bwd} >= {("bwd_vec", 8, X.BF16), ("bwd_vec", 32, X.BF16), ("bwd_vec", 4, X.F32), ("bwd_scalar", 6, X.BF16),
                                                        ("bwd_scalar", 5, X.F32)}
    assert {(c.K, c.stride) for c in bwd} >= {(3, 1), (5, 1), (7, 1), (3, 2)}
    assert {(c.dims, tuple(c.xdims)) for c in bwd if c.stride == 2} == {((5, 6, 7), (9, 11, 13)), ((7, 8, 9), (14, 16, 18))}
    assert {c.N for c in ALL} == {1, 2, 3}


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_case_is_filed_under_what_the_mirrors_and_the_library_give(c):
    from pytorch_connectomics_amd import _native as nat
    g = X.geometry(c)
    if c.has_stats:
        assert (g["slots"] > 1) == c.multi_slot, g
    assert (g["nzc"] > 1) == c.multi_chunk and g["short_last"] == c.short_last_chunk and g["ragged"] == c.ragged, g
    if c.entry in ("bwd", "bwd_add"):
        return
    if c.entry != "stem":
        assert X.mirror_variant(c) == c.variant, f"{c.id}: filed under {c.variant}, the mirror says {X.mirror_variant(c)}"
        expect = {"march": X.MARCH, "mfma": X.MFMA, "s2": X.S2, "tile": X.TILE_T, "cell": X.CELL, "generic": X.GENERIC_T, "xblock": X.XBLOCK,
                  "gather": X.GATHER, "direct": X.DIRECT}[g["form"]]
        assert expect == c.variant, f"{c.id}: dw_entry launches {g['form']}"
    try:
        for k, v in c.knobs:
            nat.check(nat.lib().pytc_set_tuning(k.encode(), int(v)), "set_tuning")
        variant, slots = X.library_variant_and_slots(c)
    finally:
        for k, v in X.KNOB_DEFAULTS.items():
            nat.check(nat.lib().pytc_set_tuning(k.encode(), int(v)), "set_tuning")
    assert variant == c.variant and slots == X.mirror_slots(c), (variant, slots, X.mirror_slots(c))


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_exactness_premises(c):
    d = X.data(c)
    x, w = d["x"], d["w"]
    assert x.abs().max() <= 4 and w.abs().max() <= 4 and torch.equal(x, x.round()) and torch.equal(w, w.round())
    for t in (x, w) + ((d["res"],) if d["res"] is not None else ()):          # storage-type operands: exact in bf16, f16 and fp32
        assert torch.equal(t.to(X.BF16).double(), t) and torch.equal(t.half().double(), t)
    if d["bias"] is not None:                                                  # (an fp32 operand)
        assert torch.equal(d["bias"] * 4, (d["bias"] * 4).round()) and torch.equal(d["bias"].float().double(), d["bias"])
        if c.entry == "stem":                                                  # the INTERIOR constant is the non-zero quarter
            k = d["bias"] + (d["w"] * d["stem_b"]).sum(0)
            assert bool((k != 0).all()) and bool((k.abs() <= 4).all()) and bool((d["stem_b"] != 0).all()) and bool((d["stem_w"] != 0).all())
        else:
            assert bool((d["bias"] != 0).all())
            big = c.out_dims[0] * c.out_dims[1] * c.out_dims[2] > 4096
            for g0 in range(0, c.C, 32):                # distinct values inside a channel group (hot channels sit on the integer / half grid)
                b = [float(v) for i, v in enumerate(d["bias"][g0:g0 + 32]) if (g0 + i) % 4 != 3]
                assert len(set(b)) >= min(len(b), 6 if big else 24), (c.id, b)
    # no two channels alike, no channel symmetric under a flip of its taps (the stem's four hot channels are two pairs of one checkerboard)
    if c.K > 1:
        assert len({tuple(col.tolist()) for col in w.t()}) == (c.C if c.entry != "stem" else c.C - 2)
        assert not bool((w == w.flip(0)).all(0).any()) or c.entry == "stem"
    # f16 in-plane sums: nine products, integers of magnitude <= 144; fp32 accumulators: multiples of 1/4 bounded by sum |x| |w| + 8
    if c.entry == "stem":
        wx, wb = d["w"] * d["stem_w"], d["w"] * d["stem_b"]
        for t in (wx, wb):
            assert torch.equal(t.half().double(), t)
        bound = float((wx.abs().sum(0) * 4 + wb.abs().sum(0) * 2 + d["bias"].abs()).max())
        assert bool((wb * 4 == (wb * 4).round()).all())
    else:
        bound = float(w.abs().sum(0).max()) * 4 + 8
        if X.form(c) == "march" and c.dtype == X.BF16 and c.knob["dwconv_march_h16"]:
            # the packed-f16 form sums the nine products of an input plane in f16, in any order: sum |x| |w| over the plane bounds every
            # partial sum; computed from the case's own x and w, per output voxel, channel and kz
            xa = d["x"].abs().permute(0, 4, 1, 2, 3)
            worst = 0.0
            for kz in range(3):
                wa = d["w"].abs()[kz * 9:(kz + 1) * 9].t().reshape(c.C, 1, 1, 3, 3)
                worst = max(worst, float(F.conv3d(xa, wa, padding=(0, 1, 1), groups=c.C).max()))
            assert 0 < worst <= 2048, f"{c.id}: a nine-product in-plane sum can reach {worst}: not exact in f16"
    assert bound * 4 < 2 ** 24
    assert torch.equal(d["y64"] * 4, (d["y64"] * 4).round())
    if c.dtype == X.F32:
        assert torch.equal(d["want"].double(), d["y64"])
    if c.has_stats:
        assert X.stats_premise_ok(d["want"])
        st = X.stats_of(d["want"])
        assert bool((d["want"].double().abs().sum((1, 2, 3)) < 2 ** 24).all()) and bool((st[:, 1] < 2 ** 24).all())
        if c.out_dims[0] * c.out_dims[1] * c.out_dims[2] > 8:
            assert bool((d["want"].float() != 0).any(1).any(1).any(1).all()), "every (sample, channel) has non-zero outputs"
    if c.nonrep:
        y, st = d["y64"], d["want"].double()
        err = (st - y).abs()
        spacing = 2.0 ** (torch.floor(torch.log2(y.abs().clamp_min(2.0 ** -60))) - 7)
        ties = int(((err == spacing / 2) & (err > 0)).sum())
        nonties = int(((err < spacing / 2) & (err > 0)).sum())
        assert ties > 0, f"{c.id}: no output that is a tie between two bf16 values"
        # without a bias or addend the sums are integers: below 512 (27 products, or the 27 that reach an output at stride 2) every
        # odd one is a tie
        if not (c.entry == "bwd" and (c.K == 3 or c.stride == 2)):
            assert nonties > 0, f"{c.id}: no non-representable output that is not a tie"
        # the range the taps can reach: 8 taps (K = 3 transposed / stride-2 gradient) give 128 + a quarter, everything else several hundred
        assert X.max_taps(c) == (8 if X.low_tap(c) else min(c.K ** 3, X.max_taps(c)))
        assert float(y.abs().max()) > (128 if X.low_tap(c) else 256)
        assert ties + nonties >= 2 * c.N, f"{c.id}: only {ties + nonties} outputs that bf16 cannot hold"
        trunc = _store(y.float(), X.BF16, "trunc")
        assert not torch.equal(_bits(trunc), _bits(d["want"])), "truncation must differ from round-to-nearest-even"
        if c.has_stats:                                  # stored and unrounded statistics differ, by a multiple of 1/4
            diff = X.stats_of(d["want"]) - torch.stack([y.sum((1, 2, 3)), (y * y).sum((1, 2, 3))], 1)
            assert bool((diff != 0).any())
    else:                                                # filed without: only where no output can be one
        reachable = c.dtype == X.BF16 and (X.max_taps(c) * 16 > 256 or (X.max_taps(c) == 8 and (d["bias"] is not None or d["res"] is not None)))
        assert not reachable, f"{c.id}: outputs that bf16 cannot hold are reachable here, the case must ask for them"
    # (with at most 8 taps the convolution itself is an integer <= 128, which bf16 holds: two roundings cannot differ from one there)
    if d["res"] is not None and c.nonrep and not X.low_tap(c):
        twice = (d["conv64"].to(X.BF16).double() + d["res"]).to(X.BF16)
        assert int((_bits(twice) != _bits(d["want"])).sum()) > 0, "two roundings must differ from one somewhere"


# ------------------------------------------------------------------------------------------------------------- 2. a correct kernel passes
@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_fp32_restatement_of_the_form_equals_the_reference_bit_for_bit(c):
    d = X.data(c)
    stored, st = restate(c, d)
    ok_y, ok_s = _agrees(c, d, stored, st)
    assert ok_y, f"{c.id}: output of the restated {X.form(c)} kernel differs from the reference"
    assert ok_s, f"{c.id}: statistics of the restated {X.form(c)} kernel differ from the reference"


# ------------------------------------------------------------------------------------------------------------- 3. seeded defects fail
DEFECTS = [
    # (defect, case it is run on, what must differ: y | stats | both)
    ("drop_face_tap", "march-h16-9x17x19-c32", "both"),
    ("flip_taps", "gather-bf16-c5-k3-vec1", "both"),
    ("flip_taps", "tile-3x9x9-c128", "both"),
    ("stats_unrounded", "mfma-v0-8x16x16-c32", "stats"),
    ("drop_ragged_stat_voxel", "mfma-small-8x8x9-c32", "stats"),
    ("count_front_plane", "tile-3x9x9-c64", "stats"),
    ("two_roundings", "res-8x16x16-c32", "y"),
    ("two_roundings", "bwd-vec-c8-k3-s1-add", "y"),
    ("stem_bias_outside", "stem-valu-5x6x8", "both"),
    ("stem_bias_outside", "stem-mfma-8x8x16", "both"),
    ("truncate", "xblock-c8-k3-w7", "both"),
    ("stats_unrounded", "tile-2x8x8-c64", "stats"),
    ("stats_unrounded", "cell-c8-bf16", "stats"),
    ("truncate", "tile-3x9x9-c128", "both"),
    ("truncate", "cell-c32-bf16", "both"),
    ("half_up", "tile-5x9x11-c64", "both"),
    ("half_up", "s2-9x20x31-c64", "both"),
    ("lost_cg_offset", "march-f32taps-8x16x16-c64", "both"),
    ("s2_even_tap_padded", "s2-28x16x32-c32", "both"),
]


def test_at_least_ten_distinct_defects_are_seeded():
    assert len({name for name, _, _ in DEFECTS}) >= 10
    assert {name for name, _, _ in DEFECTS} >= {"drop_face_tap", "flip_taps", "stats_unrounded", "drop_ragged_stat_voxel", "count_front_plane", "two_roundings",
                                               "stem_bias_outside", "truncate", "lost_cg_offset", "s2_even_tap_padded"}


@pytest.mark.parametrize("defect,cid,what", DEFECTS, ids=[f"{a}@{b}" for a, b, _ in DEFECTS])
def test_seeded_defect_fails_its_case(defect, cid, what):
    c = BY_ID[cid]
    d = X.data(c)
    assert _agrees(c, d, *restate(c, d)) == (True, True)
    ok_y, ok_s = _agrees(c, d, *restate(c, d, defect))
    if what in ("y", "both"):
        assert not ok_y, f"{defect} on {cid}: the output still equals the reference"
    else:
        assert ok_y, f"{defect} on {cid} is a statistics-only defect"
    if what in ("stats", "both"):
        assert not ok_s, f"{defect} on {cid}: the statistics still equal the reference"


def test_knob_defaults_equal_the_registry_of_the_library():
    """stencil_exact_cases.KNOB_DEFAULTS is what the GPU file restores after a case: it must be the default column of PYTC_KNOBS"""
    import re
    text = (Path(__file__).resolve().parent.parent / "pytorch_connectomics_amd" / "csrc" / "pytc_common.h").read_text()
    rows = {m.group(1): int(eval(m.group(2), {"__builtins__": {}})) for m in re.finditer(r"^\s*X\((\w+),\s*([^,]+),\s*\"", text, re.M)}
    assert len(rows) >= 20
    for k, v in X.KNOB_DEFAULTS.items():
        assert rows.get(k) == v, f"knob {k}: default {rows.get(k)} in pytc_common.h, {v} in KNOB_DEFAULTS"
    assert set(X.KNOB_DEFAULTS) == {k for k in rows if k.startswith("dwconv")}, "a depthwise knob the case table does not know"


def test_decode_names_the_geometry():
    c = BY_ID["mfma-v0-11x17x16-c32"]
    s = X.decode(c, (0, 6, 16, 8, 5))
    assert "z-chunk 1 of 2" in s and "footprint (y 2, x 1)" in s and "channel group 0" in s and "seam side y first" in s
    s = X.decode(BY_ID["tile-3x9x9-c64"], (1, 0, 17, 16, 3))
    assert "front face yes" in s and "tile (z 0, y 1, x 1)" in s
    s = X.decode(BY_ID["s2-29x9x17-c32"], (0, 14, 4, 8, 0))
    assert "z-chunk 1 of 2" in s
    assert "border yes" in X.decode(BY_ID["stem-mfma-8x8x16"], (0, 0, 3, 3, 0))

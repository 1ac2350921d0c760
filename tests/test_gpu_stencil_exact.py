"""The depthwise stencil and resampling kernels against fp64 references with NO tolerance (tests/stencil_exact_cases.py): integer operands
and quarter biases make every product, every partial sum in any order, and every GroupNorm statistic exact in fp32 (and the nine-tap
in-plane sums exact in f16), so each kernel form -- direct, K = 3 / 5 / 7 gather, x-block, the z-march on the VALU (packed-f16 partial
sums, fp32 taps, fp32 storage) and on the matrix cores (variants 0..3, small planes, storing and statistics-only launches), its gradient
entries (dwconv3d_res: ONE rounding of conv + res; pytc_dwconv3d_fwd_wide: operands scaled by 2^-40 come back exactly scaled), the
stride-2 march, the transposed cell / generic / tile forms, both stem forms and the data-gradient kernels -- must reproduce the
reference BIT FOR BIT: the output over the whole tensor, the statistics per slot and in total.

Each case calls the C ABI the way hip_ops does.  The input lies inside a NaN-filled buffer (a read past either end that reaches an
accumulator shows), the output and the statistics are views inside NaN-filled buffers with guard words on both sides (an element or slot
the kernel does not write stays NaN, a stray write changes a guard).  Every case asserts that the library's kernel variant and slot count
equal the mirror's and the value the case is filed under, runs twice and must repeat bit for bit; with N > 1 the last sample run ALONE
must give the same output and the same per-slot statistics as in the batch (batch-invariant windows); the statistics-only launch of
the matrix-core and transposed K = 3 forms must give the storing launch's statistics.  The plain wrappers (ops.dwconv3d,
ops.dwconv3d_res, ops.stem_dwconv3d, ops.dwconv3d_bwd_data) run once per form on the same operands.  Knobs are set through
ops.set_tuning inside try / finally, which restores the defaults of csrc/pytc_common.h.

What these cases cannot see is listed in DESIGN.md 4.12c (masks that are redundant with zero staging, the +-6e4 clamp of the f16 form,
the low weight halves of the matrix-core form, which are zero for integer taps).  The host test (test_host_stencil_exact_cases.py)
proves the premises and that eleven seeded defects each fail; profiles/stencil_exact_seeded_defects.txt records nine defects put into
the kernels themselves and the cases of this file that went red.

A mismatch message names the count and the first elements as (n, z, y, x, c), decoded for the form under test: tile / footprint, seam
side, z-chunk, channel group (stencil_exact_cases.decode).  The whole file takes about 10 s on an MI355X, most of it the CPU
references; the largest cases ((29, 64, 64) x 32, the (256, 64, 64) stem) about 1 s each."""
import contextlib
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import stencil_exact_cases as X  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096          # elements either side of every tensor the kernels read or write


def _ops():
    from pytorch_connectomics_amd import _native as nat, hip_ops as ops
    return nat, ops


def _ids(cs):
    return [c.id for c in cs]


@contextlib.contextmanager
def _knobs(c):
    """the case's knobs for the launches inside; afterwards the defaults (the library has no getter: the host test asserts that
    stencil_exact_cases.KNOB_DEFAULTS equals the default column of PYTC_KNOBS in csrc/pytc_common.h, for every dwconv* knob there is)"""
    _, ops = _ops()
    try:
        for k, v in c.knobs:
            ops.set_tuning(k, v)
        yield
    finally:
        for k, v in X.KNOB_DEFAULTS.items():
            ops.set_tuning(k, v)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _guarded(shape, dtype, fill=None):
    """(view of `shape`, whole buffer): the view sits GUARD elements inside a NaN-filled buffer; fill: the tensor to place in it"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    v = buf[GUARD:GUARD + n].view(tuple(shape))
    if fill is not None:
        v.copy_(fill.to(dtype))
    return v, buf


def _guards_intact(buf, what):
    fresh = torch.full((GUARD,), float("nan"), dtype=buf.dtype, device=DEV)
    assert torch.equal(_bits(buf[:GUARD]), _bits(fresh)), f"{what}: wrote BEFORE the tensor"
    assert torch.equal(_bits(buf[-GUARD:]), _bits(fresh)), f"{what}: wrote PAST the tensor"


def _check(c, got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    """torch.equal over the whole (N, D, H, W, C) tensor; on failure the count and the first differing elements, decoded"""
    got = got.cpu()
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), f"{what}: {got.dtype} {tuple(got.shape)}"
    if torch.equal(got, want):
        return
    bad = (got != want) | got.isnan()
    idx = bad.nonzero()
    first = [f"{tuple(i.tolist())} got {float(got[tuple(i)])} want {float(want[tuple(i)])} [{X.decode(c, i.tolist())}]" for i in idx[:6]]
    raise AssertionError(f"{what}: {len(idx)} of {got.numel()} elements differ (exact inputs: none may); channels "
                         f"{sorted(set(idx[:, 4].tolist()))[:16]}; first (n, z, y, x, c): " + "; ".join(first))


def _check_stats(c, st: torch.Tensor, want_y: torch.Tensor, what: str) -> None:
    """per-slot partials and their fp64 sum over slots against the statistics of the STORED reference tensor, exactly"""
    st = st.cpu().double()
    unwritten = st.isnan()
    assert not bool(unwritten.any()), (f"{what}: {int(unwritten.sum())} statistics words were not written "
                                       f"(slots {sorted(set(unwritten.nonzero()[:, 1].tolist()))[:8]})")
    total, want_total = st.sum(1), X.stats_of(want_y)
    if not torch.equal(total, want_total):
        idx = (total != want_total).nonzero()
        first = [(tuple(i.tolist()), float(total[tuple(i)]), float(want_total[tuple(i)])) for i in idx[:6]]
        raise AssertionError(f"{what}: {len(idx)} of {total.numel()} statistics differ from those of the stored tensor; first (n, sum | sumsq, c), "
                             f"got, want: {first}")
    slots = X.slot_stats(c, want_y)
    if not torch.equal(st, slots):
        idx = (st != slots).nonzero()
        first = [(tuple(i.tolist()), float(st[tuple(i)]), float(slots[tuple(i)])) for i in idx[:6]]
        raise AssertionError(f"{what}: totals agree but {len(idx)} per-slot partials differ from the mirror's slot map; first (n, slot, sum | sumsq, "
                             f"c), got, want: {first}")


def _dt(c):
    nat, _ = _ops()
    return nat.BF16 if c.dtype == X.BF16 else nat.F32


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _i3(v):
    return (C.c_int32 * 3)(*[int(a) for a in v])


class _Operands:
    """device operands of a case for samples [n0, n0 + N): the input inside its NaN buffer, taps, bias, residual / addend"""

    def __init__(self, c, d, n0=0, N=None):
        _, ops = _ops()
        self.N = c.N - n0 if N is None else N
        sl = slice(n0, n0 + self.N)
        scale = X.WIDE_SCALE if c.entry == "wide" else 1.0
        xin = d["x"][sl] * scale
        if c.entry == "stem":
            self.x, self.xbuf = _guarded((self.N,) + c.dims + (1,), torch.float32, xin.unsqueeze(-1))
            f = lambda t: t.float().contiguous().to(DEV)                  # noqa: E731
            self.packed = ops.stem_dwconv3d_pack(f(d["stem_w"]), f(d["stem_b"]), f(d["w"]), f(d["bias"]))
        else:
            self.x, self.xbuf = _guarded(xin.shape, c.dtype, xin)
        self.w = d["w"].float().contiguous().to(DEV)
        self.bias = (d["bias"] * scale).float().to(DEV) if d["bias"] is not None else None
        self.res = d["res"][sl].to(c.dtype).contiguous().to(DEV) if d["res"] is not None else None


def _launch(c, o: _Operands, store=True):
    """one call of the C ABI -> (y view | None, y buffer | None, statistics view | None, statistics buffer | None)"""
    nat, _ = _ops()
    lib = nat.lib()
    D, H, W = c.dims
    y = ybuf = st = sbuf = None
    if store:
        y, ybuf = _guarded((o.N,) + c.out_dims + (c.C,), c.dtype)
    if c.has_stats:
        slots = X.library_variant_and_slots(c)[1]
        st, sbuf = _guarded((o.N, slots, 2, c.C), torch.float32)
    if c.entry == "stem":
        wx, wb, cst, image = o.packed
        nat.check(lib.pytc_stem_dwconv3d_fwd(_p(o.x), _p(wx), _p(wb), _p(cst), _p(image), _p(y), _p(st), o.N, D, H, W, c.C, _stream()), c.id)
    elif c.entry in ("bwd", "bwd_add"):
        if c.entry == "bwd_add":
            nat.check(lib.pytc_dwconv3d_bwd_data_add(_p(o.x), _p(o.w), _p(o.res), _p(y), o.N, _i3(c.xdims), _i3(c.dims), c.C, c.K, c.stride, _dt(c),
                                                     _stream()), c.id)
        else:
            nat.check(lib.pytc_dwconv3d_bwd_data(_p(o.x), _p(o.w), _p(y), o.N, _i3(c.xdims), _i3(c.dims), c.C, c.K, c.stride, _dt(c), _stream()), c.id)
    elif c.entry == "res":
        nat.check(lib.pytc_dwconv3d_fwd_res(_p(o.x), _p(o.res), _p(y), _p(o.w), _p(o.bias), o.N, D, H, W, c.C, c.K, c.stride, _dt(c), _stream()), c.id)
    elif c.entry == "wide":
        nat.check(lib.pytc_dwconv3d_fwd_wide(_p(o.x), _p(y), _p(o.w), _p(o.bias), None, o.N, D, H, W, c.C, c.K, c.stride, _dt(c), _stream()), c.id)
    elif c.transposed:
        nat.check(lib.pytc_dwconvT3d_fwd(_p(o.x), _p(y), _p(o.w), _p(o.bias), _p(st), o.N, D, H, W, c.C, c.K, _dt(c), _stream()), c.id)
    else:
        nat.check(lib.pytc_dwconv3d_fwd(_p(o.x), _p(y), _p(o.w), _p(o.bias), _p(st), o.N, D, H, W, c.C, c.K, c.stride, _dt(c), _stream()), c.id)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                  # a GPU fault: nothing more is launched on this device in this session
        pytest.exit(f"{c.id}: the launch faulted ({e}); stopping the session", returncode=3)
    if ybuf is not None:
        _guards_intact(ybuf, f"{c.id} output")
    if sbuf is not None:
        _guards_intact(sbuf, f"{c.id} statistics")
    return y, st


def _wrapper(c, d, o: _Operands):
    """the plain hip_ops wrapper of the case's entry on the same operands -> (y, statistics | None); ops.dwconv3d_res: see _exact"""
    _, ops = _ops()
    x = o.x.clone()
    if c.entry == "stem":
        return ops.stem_dwconv3d(x, o.packed)
    if c.entry in ("bwd", "bwd_add"):
        return ops.dwconv3d_bwd_data(x, o.w, c.xdims, K=c.K, stride=c.stride, add=o.res), None
    y, st = ops.dwconv3d(x, o.w, o.bias, K=c.K, stride=c.stride, stats=c.entry == "fwd", transposed=c.transposed, wide_range=c.entry == "wide")
    return y, st


def _first_of_each_form():
    seen, out = set(), set()
    for c in X.all_cases():
        key = (c.group, X.form(c), c.dtype, c.entry, c.knobs)
        if key not in seen:
            seen.add(key)
            out.add(c.id)
    return out


WRAPPED = _first_of_each_form()


def _exact(c):
    d = X.data(c)
    want = d["want"] if c.entry != "wide" else (d["want"].double() * X.WIDE_SCALE).to(c.dtype)
    if c.entry == "wide":                      # the scaling is by a power of two: exact, and far below the f16 range
        assert torch.equal(want.double(), d["want"].double() * X.WIDE_SCALE) and float(want.abs().max()) < 2.0 ** -30
    g = X.geometry(c)
    with _knobs(c):
        variant, slots = X.library_variant_and_slots(c)
        if c.entry not in ("bwd", "bwd_add"):
            assert variant == c.variant == (X.mirror_variant(c) if c.entry != "stem" else -1), f"{c.id}: library variant {variant}, filed under {c.variant}"
            assert slots == X.mirror_slots(c), f"{c.id}: the library writes {slots} slots, the mirror says {X.mirror_slots(c)}"
        if c.has_stats:
            assert (slots > 1) == c.multi_slot
        assert (g["nzc"] > 1) == c.multi_chunk and g["short_last"] == c.short_last_chunk and g["ragged"] == c.ragged, g
        o = _Operands(c, d)
        y, st = _launch(c, o)
        _check(c, y, want, f"{c.id} [{g['form']}]")
        if c.has_stats:
            _check_stats(c, st, d["want"], f"{c.id} [{g['form']}] statistics")
        y2, st2 = _launch(c, o)
        assert torch.equal(_bits(y2), _bits(y)), f"{c.id}: a second run differs from the first"
        if c.has_stats:
            assert torch.equal(_bits(st2), _bits(st)), f"{c.id}: the statistics of a second run differ from the first"
        if c.stats_only:                       # the statistics-only launch: nothing stored, the storing launch's statistics bit for bit
            _, st3 = _launch(c, o, store=False)
            assert torch.equal(_bits(st3), _bits(st)), f"{c.id}: the statistics-only launch differs from the storing launch"
            _check_stats(c, st3, d["want"], f"{c.id} [{g['form']}] statistics-only launch")
        if c.N > 1:                            # the last sample alone: same output, same per-slot statistics as in the batch
            o1 = _Operands(c, d, n0=c.N - 1, N=1)
            y1, st1 = _launch(c, o1)
            assert torch.equal(_bits(y1), _bits(y[c.N - 1:])), f"{c.id}: sample {c.N - 1} alone differs from the same sample in the batch"
            if c.has_stats:
                assert torch.equal(_bits(st1), _bits(st[c.N - 1:])), f"{c.id}: per-slot statistics of sample {c.N - 1} depend on the batch"
        if c.id in WRAPPED:
            if c.entry == "res":
                _, ops = _ops()
                assert ops.dwconv3d_res_supported(o.x, c.K)
                # the wrapper has no bias argument: fold the (quarter) bias into the residual, which stays exact in bf16 only where it is
                # small -- so run it bias-free against its own reference: conv + res rounded once
                yw = ops.dwconv3d_res(o.x.clone(), o.w, o.res, K=c.K)
                want_w = (d["conv64"] - d["bias"] + d["res"]).to(c.dtype)
                _check(c, yw, want_w, f"{c.id} through ops.dwconv3d_res")
            else:
                yw, stw = _wrapper(c, d, o)
                torch.cuda.synchronize()
                _check(c, yw, want, f"{c.id} through the hip_ops wrapper")
                if stw is not None:
                    _check_stats(c, stw, d["want"], f"{c.id} statistics through the hip_ops wrapper")


FWD = [c for c in X.all_cases() if c.group in ("direct", "gather", "xblock")]


@pytest.mark.parametrize("c", FWD, ids=_ids(FWD))
def test_direct_gather_and_xblock_forms_exact(c):
    _exact(c)


@pytest.mark.parametrize("c", X.cases("march"), ids=_ids(X.cases("march")))
def test_z_march_valu_forms_exact(c):
    assert c.knob["dwconv_mfma"] == 0
    _exact(c)


@pytest.mark.parametrize("c", X.cases("res", "wide"), ids=_ids(X.cases("res", "wide")))
def test_z_march_gradient_entries_exact(c):
    _exact(c)


@pytest.mark.parametrize("c", X.cases("mfma"), ids=_ids(X.cases("mfma")))
def test_matrix_core_form_exact_storing_and_statistics_only(c):
    _exact(c)


@pytest.mark.parametrize("c", X.cases("s2"), ids=_ids(X.cases("s2")))
def test_stride2_march_exact(c):
    _exact(c)


@pytest.mark.parametrize("c", X.cases("cell", "generic", "tile"), ids=_ids(X.cases("cell", "generic", "tile")))
def test_transposed_forms_exact(c):
    _exact(c)


@pytest.mark.parametrize("c", X.cases("stem"), ids=_ids(X.cases("stem")))
def test_stem_forms_exact(c):
    _exact(c)


@pytest.mark.parametrize("c", X.cases("bwd"), ids=_ids(X.cases("bwd")))
def test_data_gradient_exact(c):
    _exact(c)


# ------------------------------------------------------------------------------------------------------------- the consumers of the slots
FIN_SHAPES = [("mfma-v0-10x16x16-c32", 3), ("s2-9x20x31-c64", 2), ("stem-mfma-16x24x32", 2), ("xblock-c40-k3-iters2", 1)]


@pytest.mark.parametrize("cid,N", FIN_SHAPES, ids=[a for a, _ in FIN_SHAPES])
def test_groupnorm_finalize_on_exact_multi_slot_statistics(cid, N):
    """groupnorm_finalize / groupnorm_finalize_mr on slot tensors shaped like those the cases above write (8, 6, 12 and 98 slots: fewer
    and more than the 64 slot lanes of the kernel), with integer partials so that the slot sums are exact: per (n, c) an integer mean m
    and a variance v (a multiple of 1/4), S1 = m * count and S2 = (v + m^2) * count spread unevenly over the slots, all below 2^24.

    Bound, from the operation count of groupnorm_finalize_kernel with u = 2^-24 (fp32 unit roundoff), nothing measured:
      slot sums          exact (integers below 2^24)
      mean = S1 / count  exact (the quotient is the integer m);  S2 / count - mean^2 = v exact (v + m^2 and m^2 are fp32 numbers)
      s = v + eps        one rounding: relative error <= u, which moves rsqrt(s) by <= u / 2
      rstd               r0 = rsqrtf(s) with relative error e0, refined by  r0 * (1.5 - 0.5 * s * r0 * r0):  the Newton step leaves
                         1.5 e0^2 of it (<= 2^-39 for any e0 <= 2^-20; the ISA gives v_rsq_f32 one ulp) and adds three multiplies, one
                         subtraction of a value near 1/2 from 1.5 and the final multiply: <= 3 u  ->  |rstd / rsqrt(v + eps) - 1| <= 4 u
      a = gamma * rstd   one more multiply: <= 5 u
      b = beta - mean a  the product (or the fused multiply-add) and the subtraction: |b - b_exact| <= 6 u |mean a| + u |b|
    The saved mean must equal m exactly."""
    _, ops = _ops()
    c = {k.id: k for k in X.all_cases()}[cid]
    slots, Cc = X.mirror_slots(c), c.C
    count = float(c.out_dims[0] * c.out_dims[1] * c.out_dims[2])
    g = torch.Generator().manual_seed(slots * 131 + Cc)
    lim = 2 ** 23 / count                                                        # v + m^2 below it keeps S2 (and every partial sum) under 2^24
    mmax = int((lim / 2) ** 0.5)
    m = torch.randint(-mmax, mmax + 1, (N, Cc), generator=g).double()
    v = torch.randint(1, int(lim / 2) * 4, (N, Cc), generator=g).double() / 4.0
    tot = torch.stack([m * count, (v + m * m) * count], 1)                      # (N, 2, C)
    assert float(tot.abs().max()) < 2 ** 23 and torch.equal(tot, tot.round()) and mmax >= 4
    base = torch.div(tot, slots, rounding_mode="floor")
    part = base.unsqueeze(1).repeat(1, slots, 1, 1)
    part[:, 0] += tot - base * slots
    wob = torch.randint(-1000, 1001, (N, slots // 2, 2, Cc), generator=g).double()    # uneven partials: +w on one slot, -w on its partner
    part[:, 0:2 * (slots // 2):2] += wob
    part[:, 1:2 * (slots // 2):2] -= wob
    assert torch.equal(part.sum(1), tot) and float(part.abs().sum(1).max()) < 2 ** 24
    gamma = torch.randint(-8, 9, (Cc,), generator=g).double() / 4.0
    gamma = torch.where(gamma == 0, torch.ones_like(gamma), gamma)
    beta = torch.randint(-8, 9, (Cc,), generator=g).double() / 4.0
    eps32 = float(np.float32(1e-5))
    rstd64 = 1.0 / torch.sqrt(v + eps32)
    a64 = gamma * rstd64
    b64 = beta - m * a64
    u = 2.0 ** -24
    st = part.float().to(DEV)
    ab = ops.groupnorm_finalize(st, count, gamma.float().to(DEV), beta.float().to(DEV), 1e-5).cpu().double()
    ab2, mr = ops.groupnorm_finalize_mr(st, count, gamma.float().to(DEV), beta.float().to(DEV), 1e-5)
    ab2, mr = ab2.cpu().double(), mr.cpu().double()
    assert torch.equal(ab, ab2), "groupnorm_finalize and groupnorm_finalize_mr disagree"
    assert torch.equal(mr[:, 0], m), "the saved mean of an exact integer mean"
    erstd = ((mr[:, 1] / rstd64) - 1).abs().max().item()
    ea = ((ab[:, 0] / a64) - 1).abs().max().item()
    eb = ((ab[:, 1] - b64).abs() - (6 * u * (m * a64).abs() + u * b64.abs())).max().item()
    print(f"{cid}: slots {slots}, max relative error rstd {erstd / u:.2f} u, a {ea / u:.2f} u, worst b excess over its bound {eb:.3e}")
    assert erstd <= 4 * u, f"rstd off by {erstd / u:.2f} u (bound 4 u)"
    assert ea <= 5 * u, f"a = gamma * rstd off by {ea / u:.2f} u (bound 5 u)"
    assert eb <= 0, f"b = beta - mean * a exceeds 6 u |mean a| + u |b| by {eb:.3e}"

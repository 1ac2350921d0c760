"""CPU checks of tests/dense_conv_exact_cases.py: the premises that make the GPU comparison a bit-for-bit one hold for every case, and
the case table reaches -- by the library's own launch rule, pytc_conv3d_launch_plan -- every kernel form, tiles-per-workgroup count
and chunking it is meant to cover.  If someone retunes the 256 / 512 workgroup thresholds, this file fails instead of the table
drifting off a form."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import dense_conv_exact_cases as X  # noqa: E402

ALL = X.all_cases()
IDS = [c.id for c in ALL]


def _bf16_exact(t: torch.Tensor) -> bool:
    return bool(torch.equal(t.to(torch.bfloat16).double(), t.double()))


def test_table_size_and_groups():
    assert 60 <= len(ALL) <= 80, len(ALL)
    assert {c.group for c in ALL} == {"tile", "dgrad", "phase", "stencil", "thin", "gather", "strided"}
    for c in ALL:                                   # "each case is at most ~50 k voxels"
        vox = c.N * max(c.dims[0] * c.dims[1] * c.dims[2], c.out_dims[0] * c.out_dims[1] * c.out_dims[2])
        assert vox <= 50_000, (c.id, vox)


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_case_is_filed_under_the_form_the_library_launches(c):
    if c.form == X.STRIDED:
        assert c.layout in ("conv", "convT", "conv_dgrad", "convT_dgrad")
        return
    assert c.stride == (1, 1, 1)
    for pre, _bias, res in c.operands + (("none", False, False),):           # (the impulse set runs without operands)
        form, mt, kc, nchunks, G, wgs = X.launch_plan(c, pre, res)
        if c.cin == 1 and c.form == X.THIN and pre == "none" and not res:
            assert form == X.STENCIL                # (this case's impulse set, which has no pre-activation, is a stencil launch)
            continue
        assert (form, mt) == (c.form, c.mt), f"{c.id}: filed under form {c.form} MT {c.mt}, the library launches form {form} MT {mt}"
        assert wgs >= 1
        if c.form == X.TILED:
            assert kc * nchunks == c.cin and kc in (8, 16, 24, 32)
            taps = 8 if c.phase else c.taps
            assert G == (taps * kc + 31) // 32


def test_table_reaches_every_form_mt_and_chunking():
    plan = {c.id: X.launch_plan(c, c.operands[0][0], c.operands[0][2]) for c in ALL if c.form != X.STRIDED}      # (the dense set's launch)
    by = lambda pred: {plan[c.id][:2] for c in ALL if c.id in plan and pred(c)}      # noqa: E731
    plain = lambda c: c.group == "tile"                                             # noqa: E731
    # tile form at MT 4 / 2 / 1 through ops.conv3d, its data-gradient images, the phase launch
    assert by(plain) == {(X.TILED, 4), (X.TILED, 2), (X.TILED, 1)}
    assert by(lambda c: c.layout == "dgrad") == {(X.TILED, 4), (X.TILED, 1)}
    assert by(lambda c: c.layout == "dgrad_padded") == {(X.TILED, 2)}
    for layout in ("convT_phase", "conv_dgrad_phase"):
        assert by(lambda c: c.layout == layout) == {(X.TILED, 4), (X.TILED, 2), (X.TILED, 1)}, layout
    # the shapes each MT class is built around
    want = {(64, 32): 4, (128, 16): 4, (80, 16): 4, (72, 16): 4, (32, 32): 2, (24, 32): 2, (48, 16): 2, (40, 16): 2, (64, 16): 2, (64, 1): 1}
    have = {(c.cout, c.N): plan[c.id][1] for c in ALL if plain(c) and c.dims == X.BASE and c.kernel == (3, 3, 3)}
    for key, mt in want.items():
        assert have.get(key) == mt, (key, have.get(key))
    assert {c.cout for c in ALL if plain(c) and c.mt == 1} >= {8, 16}
    # C_out % 8 != 0 at each MT the rule gives it
    odd = {(c.cout, plan[c.id][1]) for c in ALL if plain(c) and c.cout % 8}
    assert odd == {(3, 1), (20, 2), (20, 1), (36, 2), (36, 1)}, odd
    # chunkings (KC, chunks) of the tile form
    chunks = {plan[c.id][2:4] for c in ALL if plain(c)}
    assert chunks == {(8, 1), (16, 1), (24, 1), (32, 1), (8, 5), (16, 3), (32, 2), (32, 4)}, chunks
    assert {c.cin for c in ALL if c.phase} >= {8, 32, 48, 64} and {c.cout for c in ALL if c.phase} >= {8, 20, 32, 64, 80}
    # kernels: 5^3 tiled at C_in 8 / 16, the gather kernel at 32; one group (fewer than the weight ring is deep) at 1^3 x 8 channels
    k5 = {c.cin: plan[c.id][0] for c in ALL if c.kernel == (5, 5, 5)}
    assert k5 == {8: X.TILED, 16: X.TILED, 32: X.GATHER}, k5
    assert {c.kernel for c in ALL if plain(c)} == {(3, 3, 3), (1, 3, 3), (3, 1, 1), (1, 1, 1), (5, 5, 5)}
    assert any(plan[c.id][4] == 1 and plan[c.id][3] == 1 for c in ALL if plain(c) and c.kernel == (1, 1, 1))
    # zero-padded last K group (taps * KC not a multiple of 32) and the full one
    pad = {c.cin: (c.taps * plan[c.id][2]) % 32 != 0 for c in ALL if plain(c) and c.kernel == (3, 3, 3)}
    assert pad[8] and pad[16] and pad[24] and not pad[32]
    assert {c.dims for c in ALL if plain(c)} == {X.BASE, (1, 1, 1), (2, 3, 5), (4, 8, 16), (3, 8, 33)}
    assert {c.dims for c in ALL if c.phase} == {X.BASE, (2, 3, 5)}
    # every (pre-activation, bias, residual) combination at every MT of the tile form
    for mt in (4, 2, 1):
        seen = {op for c in ALL if plain(c) and c.mt == mt for op in c.operands}
        assert seen == set(X.OPERAND_COMBOS), (mt, set(X.OPERAND_COMBOS) - seen)
    ph = {op[1:] for c in ALL if c.phase for op in c.operands}
    assert ph == {(False, False), (True, False), (False, True), (True, True)}
    # the other forms
    assert {(c.cout, plan[c.id][:2]) for c in ALL if c.group == "stencil" and c.id in plan} >= {(1, (0, 1)), (3, (0, 4)), (8, (0, 8)),
                                                                                             (32, (0, 32)), (40, (0, 32))}
    assert {c.cout for c in ALL if c.group == "stencil"} == {1, 3, 8, 20, 32, 36, 40, 64}
    assert {(c.stride[0], c.dtype) for c in ALL if c.group == "stencil"} == {(1, X.BF16), (1, X.F32), (2, X.BF16), (2, X.F32)}
    assert {c.cin for c in ALL if c.group == "thin"} == {1, 2, 3, 4} and by(lambda c: c.group == "thin") == {(X.THIN, 1)}
    g = [c for c in ALL if c.group == "gather"]
    assert {c.cout for c in g if c.dtype == X.F32} == {8, 36, 80} and {c.cin for c in g if c.dtype == X.BF16} >= {6, 18, 20}
    assert by(lambda c: c.group == "gather") == {(X.GATHER, 1), (X.GATHER, 2), (X.GATHER, 4)}
    s = [c for c in ALL if c.group == "strided"]
    assert {c.layout for c in s} == {"conv", "convT", "conv_dgrad", "convT_dgrad"} and {c.cout for c in s} == {8, 24, 64}
    assert {c.stride for c in s} == {(2, 2, 2), (1, 2, 2)}


def test_query_rejects_what_the_launch_rejects():
    import ctypes as C
    from pytorch_connectomics_amd import _native as nat
    out = (C.c_int64 * 6)()
    q = nat.lib().pytc_conv3d_launch_plan
    assert q(1, 4, 4, 4, 8, 8, 2, 3, 3, nat.BF16, 0, 0, 0, out) != nat.OK                  # even kernel
    assert q(1, 4, 4, 4, 12, 8, 3, 3, 3, nat.BF16, 0, 0, 1, out) != nat.OK                 # no phase plan: C_in % 8 != 0
    assert q(1, 4, 4, 4, 8, 8, 3, 3, 3, nat.F32, 0, 0, 1, out) != nat.OK                   # the phase form is bf16
    assert q(1, 4, 4, 4, 8, 8, 3, 3, 3, nat.BF16, 0, 0, 0, None) != nat.OK
    # the stencil refuses a pre-activation and a residual
    assert q(2, 5, 9, 17, 1, 16, 3, 3, 3, nat.BF16, 0, 0, 0, out) == nat.OK and out[0] == X.STENCIL
    assert q(2, 5, 9, 17, 1, 16, 3, 3, 3, nat.BF16, 1, 0, 0, out) == nat.OK and out[0] == X.THIN
    assert q(2, 5, 9, 17, 1, 16, 3, 3, 3, nat.BF16, 0, 1, 0, out) == nat.OK and out[0] == X.THIN


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_dense_premises(c):
    """operands bf16-exact, partial sums bounded far below 2^22 in quarters, and fp32 CPU arithmetic reproduces fp64 bit for bit"""
    assert X.sum_bound(c) <= 40_012 < 2 ** 22
    for combo in c.operands:
        d = X.dense_data(c, combo)
        fx = X.pre_activation(d["x"], d["ab"], d["act"])
        for name, t in (("x", d["x"]), ("f(x)", fx), ("w", d["w"]), ("bias", d["bias"]), ("res", d["res"]), ("ab", d["ab"])):
            if t is not None:
                assert _bf16_exact(t), (c.id, combo, name)
        assert float(fx.abs().max()) <= 5 and float(d["w"].abs().max()) <= 2 and bool(torch.equal(fx * 4, (fx * 4).round()))
        if combo[0] in ("relu", "affine_leaky") and d["ab"] is not None:
            assert bool((X.pre_activation(torch.zeros_like(d["x"]), d["ab"], d["act"]) != 0).any()), "f(0) != 0 somewhere"
        # the sum of magnitudes bounds every partial sum in every order
        mag = X.linear_part(c, fx.abs(), d["w"].abs())
        worst = float(mag.max()) + (4 if d["bias"] is not None else 0) + (8 if d["res"] is not None else 0)
        assert worst <= X.sum_bound(c), (c.id, worst, X.sum_bound(c))
        ref = X.reference64(c, d)
        assert tuple(ref.shape) == (c.N, c.cout) + c.out_dims and bool(torch.equal(ref * 4, (ref * 4).round()))
        # fp32 accumulation is exact: torch's fp32 CPU convolution equals the fp64 one
        d32 = {k: (v.float() if torch.is_tensor(v) else v) for k, v in d.items()}
        assert bool(torch.equal(X.reference64(c, d32).double(), ref)), c.id
        if c.dtype == X.F32:
            assert bool(torch.equal(X.reference(c, d).double(), ref))                      # fp32 cases: nothing is rounded at all
        assert float(ref.abs().max()) > 0
        if c.real:                                                                         # the padding channels hold data to ignore
            assert bool((d["x"][:, c.real[0]:] != 0).all()) and float(ref[:, c.real[1]:].abs().max()) == 0


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_impulse_premises(c):
    """footprints disjoint, every corner / seam side / input channel / reachable tap hit, weights bf16-exact and nonzero: every output is
    one weight or zero"""
    pos = X.impulse_positions(c)
    d = X.impulse_data(c)
    x, w = d["x"], d["w"]
    cin = c.real[0] if c.real else c.cin
    assert float(x.sum()) == len(pos) == len(set(p[:4] for p in pos)) and set(x.unique().tolist()) <= {0.0, 1.0}
    assert _bf16_exact(w) and float(w.abs().min()) >= 1 and float(w.abs().max()) <= 127
    # disjoint footprints: with an all-ones weight no output collects more than one impulse
    ind = x.sum(1, keepdim=True)
    one = replace_channels(c)
    cover = X.linear_part(one, ind, torch.ones(one.weight_shape, dtype=torch.float64))
    assert float(cover.max()) <= 1.0, c.id
    # ... so every output is exactly one weight or zero, exactly representable
    ref = X.reference64(c, d)
    vals = set(ref.unique().tolist())
    assert vals <= set(w.unique().tolist()) | {0.0} and len(vals) > 1
    assert bool(torch.equal(X.reference(c, d).double(), ref))
    # channels, corners, seam sides
    assert {p[4] for p in pos} == set(range(cin)), c.id
    vox = {p[1:4] for p in pos}
    D, H, W = c.dims
    for corner in ((z, y, xx) for z in (0, D - 1) for y in (0, H - 1) for xx in (0, W - 1)):
        assert corner in vox, (c.id, corner)
    for a, (n, t) in enumerate(zip(c.dims, X.TILE)):
        for v in X._axis_coords(n, t):
            assert any(p[a] == v for p in vox), (c.id, a, v)
        if n > t:
            assert {t - 1, t} <= {p[a] for p in vox}
    if min(c.dims) >= 3:
        assert any(all(0 < p[a] < c.dims[a] - 1 for a in range(3)) for p in vox), "an interior voxel"
    # every tap the geometry can reach is hit: d(sum of outputs) / d(weight) counts the (impulse, tap) pairs that land inside
    def tap_hits(xin):
        wv = torch.ones(one.weight_shape, dtype=torch.float64, requires_grad=True)
        (g,) = torch.autograd.grad(X.linear_part(one, xin, wv).sum(), wv)
        return g.reshape(-1, c.taps).sum(0)
    hit, reach = tap_hits(ind), tap_hits(torch.ones_like(ind))
    assert bool(torch.equal(hit > 0, reach > 0)), (c.id, hit.tolist(), reach.tolist())
    if min(c.dims) >= max(c.kernel):
        assert bool((hit > 0).all())


def replace_channels(c):
    """the case as a one-channel -> one-channel conv of the same geometry (footprints and taps do not depend on the channels)"""
    from dataclasses import replace
    return replace(c, cin=1, cout=1, real=(), layout="dgrad" if c.layout == "dgrad_padded" else c.layout)

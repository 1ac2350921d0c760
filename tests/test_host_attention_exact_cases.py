"""CPU checks of tests/attention_exact_cases.py: the premises that make the GPU comparison a bit-for-bit one hold for every case (every
operand bf16-exact, a plain fp32 softmax of the generated scores is exactly 1 on the member set and 0 off it), the closed-form
references agree with fp64 autograd of the formulas the tolerance tests use, and the case table reaches the instantiations and tile
edges it is meant to cover.  A failure of tests/test_gpu_attention_exact.py therefore points at the kernel."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import attention_exact_cases as X  # noqa: E402

# the data does not depend on the storage type: one case per shape
VIT = [c for c in X.vit_cases() if c.dtype == X.F32]
WIN = [c for c in X.win_cases() if c.dtype == X.F32]
SHAPES = VIT + WIN
PAIRS = [(c, k) for c in SHAPES for k in c.sets]
PAIR_IDS = [f"{c.id}-{k}" for c, k in PAIRS]


def _bf16_exact(t: torch.Tensor) -> bool:
    return bool(torch.equal(t.to(torch.bfloat16).double(), t.double()))


def test_table_reaches_every_instantiation_and_edge():
    vit, win = X.vit_cases(), X.win_cases()
    assert {(c.dtype, c.d) for c in vit} == {(dt, d) for dt in (X.F32, X.BF16) for d in (32, 64)}
    assert {(c.dtype, c.d) for c in win} == {(dt, d) for dt in (X.F32, X.BF16) for d in (16, 32)}
    for dt, d in {(c.dtype, c.d) for c in vit}:
        assert {c.N for c in vit if (c.dtype, c.d) == (dt, d)} == {1, 63, 64, 65, 127, 128, 129, 216, 512}
    for dt, d in {(c.dtype, c.d) for c in win}:
        mine = [c for c in win if (c.dtype, c.d) == (dt, d)]
        assert {c.N for c in mine} == {1, 8, 63, 64, 70, 126, 140, 343}
        assert {c.N for c in mine if any(c.shift)} == {8, 63, 64, 70, 126, 140, 343}
        assert any(c.shift == (0, 3, 3) for c in mine)
        for a in range(3):
            assert any(c.nw[a] >= 2 and c.shift[a] > 0 for c in mine), a
    for c in vit:
        assert (c.B, c.heads) == (2, 3) and c.hid & (c.hid - 1)          # hid is no power of two
    for c in win:
        assert c.images == 2 and c.heads == 3 and c.per_image >= 2
        assert all(s == min(3, w - 1) or s == 0 for s, w in zip(c.shift, c.ws))
    for n_set in ({c.N for c in vit}, {c.N for c in win}):
        for mult in (64, 128):                  # below, at and above a tile multiple
            assert any(0 < mult - n <= 2 for n in n_set) and any(0 < n - mult <= 12 for n in n_set), (mult, n_set)
        assert 64 in n_set and 1 in n_set
    assert {65, 128, 129} <= {c.N for c in vit}                # a last tile with one key after one and after two full tiles
    # more windows than bias-gradient groups (ceil(2048 / (36 tile pairs * 3 heads)) = 19): several windows per partial slot
    assert any(c.N == 343 and c.B > 19 for c in win)


@pytest.mark.parametrize("c,kind", PAIRS, ids=PAIR_IDS)
def test_operands_are_bf16_exact_and_softmax_is_zero_or_one(c, kind):
    dd = X.data(c, kind)
    assert _bf16_exact(dd["qkv"]) and _bf16_exact(dd["dout"])
    q, k, v = X.unpack_qkv(dd["qkv"], c)
    assert float(v.min()) >= 1 and float(v.max()) <= 15 and float(X.unpack_rows(dd["dout"], c).min()) >= 1
    raw = q @ k.transpose(-1, -2)
    assert float(raw.abs().max()) < 2 ** 24 and torch.equal(raw, raw.round())
    mem = dd["mem"]
    cnt = mem.sum(-1)
    assert int(cnt.min()) >= 1                                                 # no empty member set
    s = X.scores_fp32(c, dd)
    e = torch.exp(s - s.max(-1, keepdim=True).values)                          # fp32, before normalisation
    assert e.dtype == torch.float32
    assert torch.equal(e[mem], torch.ones_like(e[mem]))
    off = e[~mem]
    if c.win and any(c.shift):
        assert off.numel() == 0 or float(off.max()) <= 1e-43                   # expf(-100): a denormal, absorbed by the row sum
        assert torch.equal(e.sum(-1), cnt.float())
    else:
        assert torch.equal(off, torch.zeros_like(off))
    # the members' score is the maximum by more than 104 over every key that is to vanish exactly
    gap = (s.max(-1, keepdim=True).values - s)
    vanish = ~mem if not c.win else ~mem & ~(dd["code_only"] & dd["table_ok"])
    assert vanish.sum() == 0 or float(gap[vanish].min()) >= 104.0
    if kind.startswith("selector") or kind.startswith("rescale"):
        assert int(cnt.max()) == 1
    if c.win:
        assert bool(mem.diagonal(dim1=-2, dim2=-1).all())                      # i itself is always a member
        t = dd["table"]
        assert set(t.unique().tolist()) <= {0.0, X.TABLE_OFF} and float(t[X.SELF_ROW].abs().max()) == 0


@pytest.mark.parametrize("c", VIT, ids=[c.id for c in VIT])
def test_selector_map_and_rescale_arrangement(c):
    nt = -(-c.N // X.TILE)
    for kind in [k for k in c.sets if not k.startswith("group")]:
        dd = X.data(c, kind)
        fac = X.tile_factors(c.N, kind)
        for s in range(c.slices):
            t = dd["tgt"][s]
            chosen = torch.bincount(t, minlength=c.N)
            assert bool((fac[t] == fac.max()).all())                           # targets live where the factor is largest
            last = int((fac == fac.max()).nonzero().max())
            assert chosen[last] >= 1
            if c.N >= 8:
                assert int((chosen == 0).sum()) >= 1 and int(chosen.max()) >= 2
            if nt >= 2:
                tiles_of = {int(j): set() for j in t.unique()}
                for i, j in enumerate(t.tolist()):
                    tiles_of[j].add(i // X.TILE)
                assert any(len(v) >= 2 for v in tiles_of.values())             # one key chosen from different query tiles
        if kind == "selector" and c.N % X.TILE:
            assert (c.N - 1) // X.TILE == nt - 1 and bool((dd["tgt"] == c.N - 1).any())      # a key of the partial last tile
    if c.N > X.TILE:
        up, down = X.tile_factors(c.N, "rescale_up"), X.tile_factors(c.N, "rescale_down")
        per_tile = lambda f: [float(f[t * X.TILE]) for t in range(nt)]        # noqa: E731
        assert per_tile(up) == sorted(per_tile(up)) and per_tile(down) == per_tile(up)[::-1] and len(set(per_tile(up))) >= 2
        # the tile maximum a row sees moves by hundreds of the scaled score at every factor step
        dd = X.data(c, "rescale_up")
        s = X.scores_fp32(c, dd)
        s = torch.where(dd["mem"], torch.full_like(s, -float("inf")), s)
        tmax = torch.stack([s[:, :, t * X.TILE:(t + 1) * X.TILE].max(-1).values for t in range(nt)], -1)
        step = (tmax[..., 1:] - tmax[..., :-1])
        f = torch.tensor(per_tile(up))
        assert float(step[..., f[1:] != f[:-1]].abs().min()) >= 200.0


def test_group_set_crosses_three_key_tiles():
    for cs in (X.vit_cases(), X.win_cases()):
        hit = False
        for c in cs:
            if c.N <= 2 * X.TILE or c.dtype != X.F32:
                continue
            mem = X.data(c, "group2")["mem"]
            tiles = torch.stack([mem[:, :, t:t + X.TILE].any(-1) for t in range(0, c.N, X.TILE)], -1).sum(-1)
            hit |= int(tiles.max()) >= 3
        assert hit


def test_swin_rows_lose_members_to_mask_alone_and_to_table_alone():
    by_mask = by_table = False
    for c in WIN:
        for kind in c.sets[1:]:
            dd = X.data(c, kind)
            by_table |= bool((dd["code_only"] & ~dd["table_ok"] & dd["label_ok"]).any())
            by_mask |= bool((dd["code_only"] & dd["table_ok"] & ~dd["label_ok"]).any())
            if any(c.shift) and c.N >= 63 and kind == "group2":
                assert bool((dd["code_only"] & dd["table_ok"] & ~dd["label_ok"]).any()), c.id
                assert bool((dd["code_only"] & ~dd["table_ok"] & dd["label_ok"]).any()), c.id
    assert by_mask and by_table


def _close(got, ref, what):
    err = float((got - ref).abs().max())
    assert err <= 1e-12 * max(1.0, float(ref.abs().max())), (what, err)


@pytest.mark.parametrize("c,kind", PAIRS, ids=PAIR_IDS)
def test_closed_forms_agree_with_fp64_autograd(c, kind):
    dd = X.data(c, kind)
    qkv = dd["qkv"].clone().requires_grad_(True)
    if c.win:
        table = dd["table"].clone().requires_grad_(True)
        o = X.win_attn_ref(qkv, table, c.B, c.heads, c.ws, c.shift, c.padded)
    else:
        o = X.attn_ref(qkv, c.B, c.heads)
    o.backward(dd["dout"])
    ref = X.backward_reference(c, dd)
    mem, (_, _, v) = dd["mem"].double(), X.unpack_qkv(dd["qkv"], c)
    _close(X.pack_rows(mem / mem.sum(-1, keepdim=True) @ v, c), o.detach(), "O")
    o_exp, m, lse64, cnt = X.forward_expected(c, dd)
    if int(cnt.max()) == 1:
        _close(o_exp.double(), o.detach(), "O (one-hot: the expected fp32 O is the exact one)")
    hid = c.hid
    for part, sl in (("dQ", slice(0, hid)), ("dK", slice(hid, 2 * hid)), ("dV", slice(2 * hid, 3 * hid))):
        _close(ref["dqkv"][:, sl], qkv.grad[:, sl], part)
    if c.win:
        _close(ref["dtable"], table.grad, "dtable")
        used = torch.zeros(2197, dtype=torch.bool)
        used[X._rel(c.N).reshape(-1)] = True
        assert float(ref["dtable_abs"][~used].abs().sum()) == 0
    if int(cnt.max()) == 1:                                                    # one-hot sets: what the GPU test asserts exactly
        assert float(ref["dqkv"][:, :2 * hid].abs().max()) == 0
        assert torch.equal(ref["dqkv"], ref["dqkv"].round())
        if c.win:
            assert float(ref["dtable"].abs().max()) == 0
    # the log-sum-exp of the same scores in fp64
    s64 = X.scores_fp32(c, dd).double()
    lse_ref = torch.logsumexp(s64, -1).reshape(lse64.shape)
    assert bool(((lse64 - lse_ref).abs() <= 1e-12 * lse_ref.abs().clamp_min(1.0)).all())
    if int(cnt.max()) > 1:
        assert float(lse64.abs().max()) < 2048                                 # (the magnitude grad_tolerance's docstring quotes)


def test_gradient_bound_is_small_next_to_one_wrong_member():
    """the derived bound must stay well below the effect the group set is there to see: one member more or less in a row moves its
    elements by about 1 / |M| of their size (|M| <= 256)"""
    for c in VIT + WIN:
        for kind in [k for k in c.sets if k.startswith("group")]:
            dd = X.data(c, kind)
            _, _, lse64, cnt = X.forward_expected(c, dd)
            rel = float(X.ulp32(lse64.abs().max())) + (float(cnt.max()) + c.d + 32) * X.EPS32
            assert rel <= 2.0 ** -12 and rel * float(cnt.max()) <= 0.05, (c.id, kind, rel)


@pytest.mark.parametrize("c", X.gemm_cases(), ids=[c.id for c in X.gemm_cases()])
def test_gemm_cases_are_exact_integers(c):
    dd = X.gemm_data(c)
    for k, t in dd.items():
        if t is not None:
            assert _bf16_exact(t) and float(t.abs().max()) <= 3, k
    ref = X.gemm_reference(c, dd)
    for k, t in ref.items():
        assert torch.equal(t, t.round()) and float(t.abs().max()) < 2 ** 24, k
        assert torch.equal(t.float().double(), t)
    assert (c.P > 0) == ("dpos" in ref)


def test_gemm_table():
    cs = X.gemm_cases()
    assert {(c.M, c.K, c.N) for c in cs} == {(1, 48, 48), (65, 48, 144), (437, 80, 33), (128, 32, 64), (130, 4096, 48)}
    assert {c.P for c in cs if c.K == 4096} == {65}
    assert any(c.K % 32 for c in cs) and any(c.M == 1 for c in cs) and any(c.N < 64 for c in cs)

"""Memory footprint of every backward launch of the training step, under guard bands (tests/train_footprint_cases.py).

The cases go through nat.lib() with raw pointers, not through the hip_ops wrappers (which allocate results and slot workspaces with
torch.empty, next to whatever the caching allocator holds).  Every buffer -- operand, output, workspace -- is one allocation
[guard | payload | guard] with 4096 elements per guard; guards and the payloads of outputs and workspaces are filled with a NaN of a
recognisable payload that is compared by bits.  Each case runs at the natural alignment and with every payload shifted off it: by one
element for the scalar element-wise kernels (pytc_gelu, pytc_add_inplace, pytc_grn_bwd_apply), by 16 bytes for everything else.  The 16
bytes are this harness's choice, not a rule of include/pytc_hip.h (which states no alignment for these entries, and the entries check
none): most of these launches move 16-byte vectors, one case walks vector and scalar kernels through its knob forms with the same
buffers, and 16 bytes is what every slice the hip_ops wrappers hand out keeps.  The scalar forms among them (the generic fp32
pw_wgrad kernel, the thin operand, bf16 C = 12 in norm_bwd) would admit one element; they are not run that way here.  No buffer is ever
smaller than the header demands: workspace sizes come from the library's own queries.

After every launch: status PYTC_OK; every guard bit-identical to its fill; every operand bit-identical to its copy; no sentinel left in
any output; every output equal to the fp64 reference; *slots_out x (nW + nB) inside the queried size; the documented partial regions
free of sentinels and -- summed over their slots on the host in fp64 -- equal to the reference (no offset arithmetic of hip_ops.py is
used: the regions come from train_footprint_cases.regions); what the header does NOT document as written (the bias region without
want_db, the term region at sps == 1, the workspace past *slots_out slots) still all sentinel; the partials reduced by
pytc_reduce_slots_multi (out_t 0 and > 0) equal to the reference and to the immediate form's bits; every knob form equal to the default
form's bits under the same checks.  Knobs are restored in a finally block.  The knob forms are those the launches of these families read;
`elementwise_vec` has none (train_footprint_cases.py says which launches read it).

Seeded defects this module catches are recorded in profiles/train_footprint_seeded_defects.txt, durations and the case count in
profiles/train_footprint_probe.txt."""
import contextlib
import ctypes as C
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import train_footprint_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = T.GUARD
BF16, F32 = T.BF16, T.F32


def _ops():
    from pytorch_connectomics_amd import _native as nat, hip_ops as ops
    return nat, ops


@contextlib.contextmanager
def _knobs(kn):
    _, ops = _ops()
    try:
        for k, v in kn:
            ops.set_tuning(k, int(v))
        yield
    finally:
        for k, v in T.KNOB_DEFAULTS.items():
            ops.set_tuning(k, v)


def _ibits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _sent(dtype):
    return T.SENTINEL_16 if torch.empty(0, dtype=dtype).element_size() == 2 else T.SENTINEL_F32


def _all_sentinel(v):
    return bool((_ibits(v) == _sent(v.dtype)).all())


def _sentinels_in(v):
    return int((_ibits(v) == _sent(v.dtype)).sum())


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Arena:
    """the buffers of one launch: [guard | payload | guard] each, payload at the natural or at the weakest admitted alignment"""

    def __init__(self, weak: bool):
        self.weak = weak
        self.bufs = []           # (name, whole buffer, payload start, payload elements, operand copy | None)

    def _new(self, name, n, dtype, weak_bytes):
        esz = torch.empty(0, dtype=dtype).element_size()
        shift = max(1, weak_bytes // esz) if self.weak else 0
        buf = torch.empty((n + 2 * GUARD + shift,), dtype=dtype, device=DEV)
        _ibits(buf).fill_(_sent(dtype))
        lo = GUARD + shift
        v = buf[lo:lo + n]
        assert v.data_ptr() % (weak_bytes if self.weak else 256) == 0 and (not self.weak or v.data_ptr() % (2 * weak_bytes) != 0)
        return buf, lo, v

    def operand(self, name, t, weak_bytes=16):
        if t is None:
            return None
        t = t.to(DEV).contiguous()
        buf, lo, v = self._new(name, t.numel(), t.dtype, weak_bytes)
        v.copy_(t.reshape(-1))
        self.bufs.append((name, buf, lo, t.numel(), v.clone()))
        return v.view(t.shape)

    def output(self, name, shape, dtype, weak_bytes=16, init=None):
        n = 1
        for s in shape:
            n *= int(s)
        buf, lo, v = self._new(name, n, dtype, weak_bytes)
        if init is not None:
            v.copy_(init.to(DEV).reshape(-1))
        self.bufs.append((name, buf, lo, n, None))
        return v.view(tuple(int(s) for s in shape))

    def check(self, what):
        for name, buf, lo, n, copy in self.bufs:
            assert _all_sentinel(buf[:lo]), f"{what}: wrote BEFORE {name}"
            assert _all_sentinel(buf[lo + n:]), f"{what}: wrote PAST {name}"
            if copy is not None:
                assert torch.equal(_ibits(buf[lo:lo + n]), _ibits(copy)), f"{what}: operand {name} changed"


def _ok(st, what):
    nat, _ = _ops()
    torch.cuda.synchronize()
    msg = nat.lib().pytc_last_error()
    assert st == nat.OK, f"{what}: status {st}: {msg.decode() if msg else '?'}"


def _check_out(what, name, got, ref: T.Ref, res):
    assert got.dtype == ref.dtype and got.numel() == ref.ref.numel(), f"{what} {name}: {got.dtype} {tuple(got.shape)}"
    left = _sentinels_in(got)
    assert left == 0, f"{what} {name}: {left} of {got.numel()} elements were never written"
    want = ref.ref.to(DEV).reshape(got.shape)
    if ref.ulp == 0:
        bad = got.double() != want
        assert not bool(bad.any()), f"{what} {name}: {int(bad.sum())} of {got.numel()} elements differ from fp64, max |diff| " \
                                    f"{float((got.double() - want).abs().max())}"
    else:
        assert bool(torch.isfinite(got.float()).all()), f"{what} {name}: non-finite"
        d = T.ulp_distance(got, want.to(ref.dtype))
        print(f"[{what}] {name}: {int((d > 0).sum())} of {d.numel()} elements one unit off the once-rounded fp64 value")
        assert int(d.max()) <= ref.ulp, f"{what} {name}: {int((d > ref.ulp).sum())} elements more than {ref.ulp} ulp off, max {int(d.max())}"
    res[name] = got.clone()


def _code(dt):
    nat, _ = _ops()
    return nat.BF16 if dt == BF16 else nat.F32


def _check_regions(what, c, ws, S, res, empty=()):
    """the documented regions of `ws` for S slots: written ones without a sentinel and summing to the reference, the others and
    the tail of the workspace untouched; empty: slot indices that received no row and must hold zeros"""
    regs = T.regions(c, S)
    end = 0
    for r in regs:
        part = ws[r.offset:r.offset + r.slots * r.n]
        end = r.offset + r.slots * r.n
        assert end <= ws.numel(), f"{what}: region {r.name} ends at {end}, the query promised {ws.numel()} floats"
        if not r.written:
            assert _all_sentinel(part), f"{what}: region {r.name} is documented as not written here, but {part.numel() - _sentinels_in(part)} elements were"
            continue
        left = _sentinels_in(part)
        assert left == 0, f"{what}: {left} of {part.numel()} partials of region {r.name} were never written"
        tot = part.view(r.slots, r.n).double().sum(0)
        bad = tot != r.total.to(DEV)
        assert not bool(bad.any()), f"{what}: region {r.name} summed over its {r.slots} slots differs from fp64 in {int(bad.sum())} of {r.n} sums"
        if r.slots == S:
            for s in empty:
                assert not bool(part.view(r.slots, r.n)[s].any()), f"{what}: region {r.name}: slot {s} has no row but is not zero"
        res["part_" + r.name] = part.clone()
    assert _all_sentinel(ws[end:]), f"{what}: wrote past the {S} slots it reported ({ws.numel() - end - _sentinels_in(ws[end:])} floats)"
    return regs


def _reduce(what, A, ws, regs, transposed, res):
    """pytc_reduce_slots_multi over the written regions, into guarded outputs; transposed: {region name: out_t}"""
    nat, ops = _ops()
    regs = [r for r in regs if r.written]
    arr = (nat.ReduceItem * len(regs))()
    outs = []
    for i, r in enumerate(regs):
        o = A.output(f"reduced_{r.name}", (r.n,), F32)
        arr[i].part, arr[i].out, arr[i].n, arr[i].slots = ws[r.offset:].data_ptr(), o.data_ptr(), r.n, r.slots
        arr[i].out_t = transposed.get(r.name, 0)
        outs.append(o)
    _ok(nat.lib().pytc_reduce_slots_multi(arr, len(regs), ops._stream()), what + " reduce_slots_multi")
    A.check(what + " reduce_slots_multi")
    for r, o in zip(regs, outs):
        assert _sentinels_in(o) == 0, f"{what}: reduced {r.name} has unwritten elements"
        t = transposed.get(r.name, 0)
        got = o.view(t, r.n // t).t().reshape(-1) if t else o
        bad = got.double() != r.total.to(DEV)
        assert not bool(bad.any()), f"{what}: reduce_slots_multi({r.name}, out_t={t}) differs from fp64 in {int(bad.sum())} of {r.n} sums"
        res["reduced_" + r.name] = got.clone()


def _empty_slots(c, kn, S):
    """slot indices the mirrors say receive no row (default form only: the knob forms change the split)"""
    if kn or "empty_last" not in c.edges:
        return ()
    f = T.slot_facts(c)
    assert f["slots"] == S
    per, used = f["per_split"], f["used"]
    return tuple(n * per + j for n in range(S // per) for j in range(used, per))


# ------------------------------------------------------------------------------------------------------------------ the runners
def _run_pw(c, A, kn, what):
    nat, ops = _ops()
    lib, b, p, res = nat.lib(), T.build(c), dict(c.p), {}
    N, rows, ci, co, code = p["N"], p["rows"], p["c_in"], p["c_out"], _code(p["dtype"])
    nW, nB = ci * co, co
    act = nat.ACT_GELU if p["gelu"] else nat.ACT_NONE
    x, dy, ab = A.operand("x", b.inputs["x"]), A.operand("dy", b.inputs["dy"]), A.operand("ab", b.inputs.get("ab"))
    bound = lib.pytc_pw_wgrad_slots(N * rows)
    ws = A.output("workspace", (bound * (nW + nB),), F32)
    if c.entry == "pytc_pw_wgrad":
        dW = A.output("dW", (co, ci), F32)
        db = A.output("db", (co,), F32) if p["want_db"] else None
        _ok(lib.pytc_pw_wgrad(P(x), P(ab), P(dy), P(dW), P(db), P(ws), N, rows, ci, co, code, act, ops._stream()), what)
        A.check(what)
        _check_out(what, "dW", dW, b.outputs["dW"], res)
        if db is not None:
            _check_out(what, "db", db, b.outputs["db"], res)
        return res
    used = C.c_int(-1)
    if c.entry == "pytc_pw_wgrad_partial":
        st = lib.pytc_pw_wgrad_partial(P(x), P(ab), P(dy), P(ws), p["want_db"], N, rows, ci, co, code, act, C.byref(used), ops._stream())
    else:
        assert lib.pytc_pw_wgrad_dgrad_supported(ci, co, code) == 1
        wt = A.operand("w_t_paired", ops.pw_pack_weight_paired(b.inputs["w"].to(DEV), transposed=True))
        dx = A.output("dx", (N, rows, ci), BF16)
        st = lib.pytc_pw_wgrad_dgrad_partial(P(x), P(dy), P(wt), P(dx), P(ws), p["want_db"], N, rows, ci, co, code, C.byref(used), ops._stream())
    _ok(st, what)
    A.check(what)
    S = used.value
    assert 1 <= S and S * (nW + nB) <= ws.numel(), f"{what}: *slots_out = {S} does not fit the {bound} slots the query sized"
    assert S == T.launch_slots(c, kn), f"{what}: the library wrote {S} slots, the mirror says {T.launch_slots(c, kn)}"
    if c.entry == "pytc_pw_wgrad_dgrad_partial":
        _check_out(what, "dx", dx, b.outputs["dx"], res)
    regs = _check_regions(what, c, ws, S, res, _empty_slots(c, kn, S))
    _reduce(what, A, ws, regs, {"dW": ci}, res)
    # the immediate form's bits
    ws2 = A.output("workspace_imm", (bound * (nW + nB),), F32)
    dW = A.output("dW_imm", (co, ci), F32)
    db = A.output("db_imm", (co,), F32) if p["want_db"] else None
    _ok(lib.pytc_pw_wgrad(P(x), P(ab), P(dy), P(dW), P(db), P(ws2), N, rows, ci, co, code, act, ops._stream()), what + " immediate")
    A.check(what + " immediate")
    assert torch.equal(_ibits(dW.reshape(-1)), _ibits(res["reduced_dW"])), f"{what}: immediate dW != reduced partials"
    if db is not None:
        assert torch.equal(_ibits(db), _ibits(res["reduced_db"])), f"{what}: immediate db != reduced partials"
    return res


def _run_mixer(c, A, kn, what):
    nat, ops = _ops()
    lib, b, p, res = nat.lib(), T.build(c), dict(c.p), {}
    N, rows, hid = p["N"], p["rows"], p["c_hid"]
    i = b.inputs
    t, ab = A.operand("t", i["t"]), A.operand("ab", i["ab"])
    if c.entry == "pytc_mixer_bwd_rc":
        gn = p["gn"]
        assert lib.pytc_mixer_bwd_rc_supported(32, hid, 32, nat.BF16) >= (2 if gn else 1)
        dy = A.operand("dy", i["dy"])
        w2p = A.operand("w2_paired", ops.pw_pack_weight_paired(i["w2"].to(DEV)))
        w3t = A.operand("w3t_paired", ops.pw_pack_weight_paired(i["w3"].to(DEV), transposed=True))
        b2 = A.operand("b2", i["b2"])
        mr = A.operand("mean_rstd", i["mr"]) if gn else None
        W2 = A.operand("W2", i["w2"]) if gn else None
        gamma = A.operand("gamma", i["gamma"]) if gn else None
        dhp = A.output("dhp", (N, rows, hid), BF16)
        s_out = A.output("s_out", (N, 2, 32), F32) if gn else None
        coef = A.output("coef", (N, 3, 32), F32) if gn else None
        n_ws = int(lib.pytc_mixer_bwd_rc_ws_elems(N, rows, hid, gn))
        ws = A.output("workspace", (n_ws,), F32)
        used = C.c_int(-1)
        _ok(lib.pytc_mixer_bwd_rc(P(t), P(ab), P(mr), P(dy), P(w2p), P(b2), P(w3t), P(W2), P(gamma), float(i.get("count", 0.0)), P(dhp), P(ws),
                                  P(s_out), P(coef), p["want_db3"], gn, N, rows, 32, hid, 32, nat.BF16, C.byref(used), ops._stream()), what)
        A.check(what)
        S = used.value
        assert S == N * lib.pytc_mixer_bwd_rc_sps(N, rows, hid) == T.launch_slots(c, kn), f"{what}: *slots_out = {S}"
        _check_out(what, "dhp", dhp, b.outputs["dhp"], res)
    else:
        gn, Cc = 1, p["c"]
        assert lib.pytc_pw_wgrad_groupnorm_supported(Cc, hid, nat.BF16)
        mr, dh = A.operand("mean_rstd", i["mr"]), A.operand("dhp", i["dhp"])
        W2, gamma = A.operand("W2", i["w2"]), A.operand("gamma", i["gamma"])
        s_out, coef = A.output("s_out", (N, 2, Cc), F32), A.output("coef", (N, 3, Cc), F32)
        n_ws = int(lib.pytc_pw_wgrad_groupnorm_ws_elems(N, rows, Cc, hid))
        ws = A.output("workspace", (n_ws,), F32)
        _ok(lib.pytc_pw_wgrad_groupnorm(P(t), P(mr), P(ab), P(dh), P(W2), P(gamma), float(i["count"]), P(s_out), P(coef), P(ws), N, rows, Cc,
                                        hid, nat.BF16, ops._stream()), what)
        A.check(what)
        S = N * lib.pytc_pw_wgrad_groupnorm_sps(N, rows, Cc, hid)
        assert S == T.launch_slots(c, kn), f"{what}: {S} slots, the mirror says {T.launch_slots(c, kn)}"
    if gn:
        _check_out(what, "s_out", s_out, b.outputs["s_out"], res)
        _check_out(what, "coef", coef, b.outputs["coef"], res)
    regs = _check_regions(what, c, ws, S, res, _empty_slots(c, kn, S))
    assert regs[-1].offset + regs[-1].slots * regs[-1].n == n_ws, f"{what}: the regions do not fill the {n_ws} floats of the query"
    _reduce(what, A, ws, regs, {}, res)
    return res


def _run_norm(c, A, kn, what):
    nat, ops = _ops()
    lib, b, p, res = nat.lib(), T.build(c), dict(c.p), {}
    N, rows, Cc, dt = p["N"], p["rows"], p["C"], p["dtype"]
    i = b.inputs
    dtn, t, mr, gamma = A.operand("dtn", i["dtn"]), A.operand("t", i["t"]), A.operand("mean_rstd", i["mr"]), A.operand("gamma", i["gamma"])
    if c.entry == "pytc_norm_bwd_apply":
        s_in = A.operand("s_in", i["s_in"])
        crop = ops._i3(p["grid"]) if p["crop"] else None
        D, H, W = p["grid"]
        out_rows = (D - 1) * (H - 1) * (W - 1) if p["crop"] else rows
        out = A.output("dt", (N, out_rows, Cc), dt)
        _ok(lib.pytc_norm_bwd_apply(P(dtn), P(t), P(mr), P(gamma), P(s_in), p["s_parts"], P(out), N, rows, Cc, float(i["count"]), _code(dt),
                                    crop, ops._stream()), what)
        A.check(what)
        _check_out(what, "dt", out, b.outputs["dt"], res)
        return res
    n_ws = lib.pytc_norm_bwd_ws_elems(N, rows, Cc)
    slots = T.launch_slots(c)
    assert n_ws == N * slots * 2 * Cc and slots > 1
    ws = A.output("stats_ws", (n_ws,), F32)
    s_out = A.output("s_out", (N, 2, Cc), F32)
    if c.entry == "pytc_norm_bwd":
        out = A.output("dt", (N, rows, Cc), dt)
        _ok(lib.pytc_norm_bwd(P(dtn), P(t), P(mr), P(gamma), P(ws), P(s_out), P(out), N, rows, float(i["count"]), Cc, _code(dt), ops._stream()), what)
    else:
        _ok(lib.pytc_norm_bwd_stats(P(dtn), P(t), P(mr), P(ws), P(s_out), N, rows, Cc, _code(dt), ops._stream()), what)
    A.check(what)
    _check_out(what, "s_out", s_out, b.outputs["s_out"], res)
    if c.entry == "pytc_norm_bwd":
        _check_out(what, "dt", out, b.outputs["dt"], res)
    left = _sentinels_in(ws)
    assert left == 0, f"{what}: {left} of {n_ws} statistics partials were never written"
    tot = ws.view(N, slots, 2 * Cc).double().sum(1)
    assert torch.equal(tot, b.totals["stats"].to(DEV)), f"{what}: the slot partials do not sum to the statistics"
    f = T.slot_facts(c)
    for s in range(f["used"], slots):
        assert not bool(ws.view(N, slots, 2 * Cc)[:, s].any()), f"{what}: slot {s} has no row but is not zero"
    res["stats_ws"] = ws.clone()
    return res


def _run_dw(c, A, kn, what):
    nat, ops = _ops()
    lib, b, p, res = nat.lib(), T.build(c), dict(c.p), {}
    N, Cc, K, st, code = p["N"], p["C"], p["K"], p["stride"], _code(p["dtype"])
    nW, nB = K ** 3 * Cc, Cc
    gd, xd = ops._i3(p["gdims"]), ops._i3(p["xdims"])
    g, x = A.operand("g", b.inputs["g"]), A.operand("x", b.inputs["x"])
    bound = lib.pytc_dw_wgrad_slots(N, gd, xd, Cc, K, st, code)
    mirror = T.launch_slots(c, kn)
    assert bound > 1 and (mirror is None or bound == mirror), f"{what}: the library sizes {bound} slots, the mirror {mirror}"
    ws = A.output("workspace", (bound * (nW + nB),), F32)
    if c.entry == "pytc_dw_wgrad":
        dW = A.output("dW", (K ** 3, Cc), F32)
        db = A.output("db", (Cc,), F32) if p["want_db"] else None
        _ok(lib.pytc_dw_wgrad(P(g), P(x), P(dW), P(db), P(ws), N, gd, xd, Cc, K, st, code, ops._stream()), what)
        A.check(what)
        _check_out(what, "dW", dW, b.outputs["dW"], res)
        if db is not None:
            _check_out(what, "db", db, b.outputs["db"], res)
        return res
    used = C.c_int(-1)
    _ok(lib.pytc_dw_wgrad_partial(P(g), P(x), P(ws), p["want_db"], N, gd, xd, Cc, K, st, code, C.byref(used), ops._stream()), what)
    A.check(what)
    S = used.value
    assert 1 <= S <= bound, f"{what}: *slots_out = {S}, the query sized {bound}"
    regs = _check_regions(what, c, ws, S, res)
    _reduce(what, A, ws, regs, {"dW": Cc}, res)
    ws2 = A.output("workspace_imm", (bound * (nW + nB),), F32)
    dW = A.output("dW_imm", (K ** 3, Cc), F32)
    db = A.output("db_imm", (Cc,), F32) if p["want_db"] else None
    _ok(lib.pytc_dw_wgrad(P(g), P(x), P(dW), P(db), P(ws2), N, gd, xd, Cc, K, st, code, ops._stream()), what + " immediate")
    A.check(what + " immediate")
    assert torch.equal(_ibits(dW.reshape(-1)), _ibits(res["reduced_dW"])), f"{what}: immediate dW != reduced partials"
    if db is not None:
        assert torch.equal(_ibits(db), _ibits(res["reduced_db"])), f"{what}: immediate db != reduced partials"
    return res


def _run_elementwise(c, A, kn, what):
    nat, ops = _ops()
    lib, b, p, res = nat.lib(), T.build(c), dict(c.p), {}
    dt = p["dtype"]
    esz = 2 if dt == BF16 else 4
    i = b.inputs
    if c.entry == "pytc_gelu":
        x, dy = A.operand("x", i["x"], esz), A.operand("dy", i.get("dy"), esz)
        out = A.output("out", (p["n"],), dt, esz)
        _ok(lib.pytc_gelu(P(x), P(dy), P(out), p["n"], _code(dt), ops._stream()), what)
    elif c.entry == "pytc_add_inplace":
        x = A.operand("x", i["x"], esz)
        out = A.output("y", (p["n"],), dt, esz, init=b.inout["y"])
        _ok(lib.pytc_add_inplace(P(out), P(x), p["n"], _code(dt), ops._stream()), what)
    elif c.entry == "pytc_copy_zero_front":
        src = A.operand("src", i["src"])
        out = A.output("dst", tuple(i["src"].shape), dt)
        _ok(lib.pytc_copy_zero_front(P(src), P(out), p["N"], ops._i3(p["dims"]), p["C"], _code(dt), ops._stream()), what)
    else:
        dh2, hp = A.operand("dh2", i["dh2"], esz), A.operand("hp", i["hp"], esz)
        Aa, Bb = A.operand("A", i["A"], 4), A.operand("B", i["B"], 4)
        out = A.output("out", tuple(i["hp"].shape), dt, esz)
        _ok(lib.pytc_grn_bwd_apply(P(dh2), P(hp), P(Aa), P(Bb), P(out), p["N"], p["rows"], p["C"], _code(dt), ops._stream()), what)
    A.check(what)
    (name, ref), = b.outputs.items()
    _check_out(what, name, out, ref, res)
    return res


def _run_dense(c, A, kn, what):
    nat, ops = _ops()
    lib, b, p, res = nat.lib(), T.build(c), dict(c.p), {}
    N, code = p["N"], _code(p["dtype"])
    i = b.inputs
    if c.entry == "pytc_conv3d_wgrad":
        ci, co, k = p["c_in"], p["c_out"], p["k"]
        taps = k[0] * k[1] * k[2]
        a, dy = A.operand("a", i["a"]), A.operand("dy", i["dy"])
        n_ws = int(lib.pytc_conv3d_wgrad_ws_elems(N, *p["dims"], ci, co, ops._i3(k), code))
        assert n_ws % (taps * co * ci) == 0 and (kn or n_ws // (taps * co * ci) > 1), f"{what}: workspace of {n_ws} floats"      # (the knob's VALU plan: one slot below 16 384 rows)
        ws, dW = A.output("workspace", (n_ws,), F32), A.output("dW", (taps, co, ci), F32)
        _ok(lib.pytc_conv3d_wgrad(P(a), P(dy), P(dW), P(ws), N, *p["dims"], ci, co, ops._i3(k), code, ops._stream()), what)
        outs = {"dW": dW}
    elif c.entry == "pytc_conv3d_wgrad_strided":
        ck, co = p["c_k"], p["c_o"]
        small = tuple((v + 1) // 2 for v in p["big"])
        big, sm = A.operand("big", i["big"]), A.operand("small", i["small"])
        n_ws = int(lib.pytc_conv3d_wgrad_strided_ws_elems(N, ops._i3(small), ck, co, ops._i3((3, 3, 3))))
        assert n_ws // (27 * ck * co) > 1, f"{what}: workspace of {n_ws} floats"
        ws, dW = A.output("workspace", (n_ws,), F32), A.output("dW", (27, co, ck), F32)
        _ok(lib.pytc_conv3d_wgrad_strided(P(big), P(sm), P(dW), P(ws), N, ops._i3(p["big"]), ops._i3(small), ck, co, ops._i3((3, 3, 3)),
                                          ops._i3((2, 2, 2)), ops._i3((1, 1, 1)), code, ops._stream()), what)
        outs = {"dW": dW}
    else:
        lo, ci, cu, ce = p["lo"], p["c_in"], p["c_u"], p["c_e"]
        rows = N * lo[0] * lo[1] * lo[2]
        x_low, d = A.operand("x_low", i["x_low"]), A.operand("d", i["d"])
        n_ws = int(lib.pytc_upcat_deconv2_wgrad_ws_elems(rows, ci, cu, code))
        assert n_ws % ((ci + 1) * 8 * cu) == 0 and n_ws // ((ci + 1) * 8 * cu) > 1, f"{what}: workspace of {n_ws} floats"
        ws, dw, db = A.output("workspace", (n_ws,), F32), A.output("dw", (ci, cu, 2, 2, 2), F32), A.output("db", (cu,), F32)
        if c.entry == "pytc_upcat_deconv2_wgrad":
            st = lib.pytc_upcat_deconv2_wgrad(P(x_low), P(d), P(ws), P(dw), P(db), N, *lo, *p["sk"], ci, ce, cu, code, ops._stream())
        else:
            st = lib.pytc_deconv2_upfirst_wgrad(P(x_low), P(d), P(ws), P(dw), P(db), N, *lo, ci, ce, cu, code, ops._stream())
        _ok(st, what)
        outs = {"dw": dw, "db": db}
    A.check(what)
    for name, o in outs.items():
        _check_out(what, name, o, b.outputs[name], res)
    return res


_RUNNERS = {"pw": _run_pw, "mixer": _run_mixer, "norm": _run_norm, "dw": _run_dw, "elementwise": _run_elementwise, "dense": _run_dense}


def _run_case(c):
    """every knob form at both alignments: the same checks, and the default form's bits"""
    first, runs = None, 0
    for kn in ((),) + c.forms:
        with _knobs(kn):
            for weak in (False, True):
                what = f"{c.id}{' ' + str(dict(kn)) if kn else ''}{' weak-aligned' if weak else ''}"
                res = _RUNNERS[c.family](c, Arena(weak), kn, what)
                runs += 1
                if first is None:
                    first = res
                    continue
                for name, v in res.items():
                    if name.startswith("part_") and v.numel() != first[name].numel():
                        continue                        # another slot count: its partials were checked against fp64 above
                    if name.startswith("part_") and kn:
                        continue
                    assert torch.equal(_ibits(v), _ibits(first[name])), f"{what}: {name} differs from the default form's bits"
    return runs


def _ids(cs):
    return [c.id for c in cs]


@pytest.mark.parametrize("c", T.by_family("pw"), ids=_ids(T.by_family("pw")))
def test_pw_wgrad_footprint(c):
    _run_case(c)


@pytest.mark.parametrize("c", T.by_family("mixer"), ids=_ids(T.by_family("mixer")))
def test_mixer_bwd_footprint(c):
    _run_case(c)


@pytest.mark.parametrize("c", T.by_family("norm"), ids=_ids(T.by_family("norm")))
def test_norm_bwd_footprint(c):
    _run_case(c)


@pytest.mark.parametrize("c", T.by_family("dw"), ids=_ids(T.by_family("dw")))
def test_dw_wgrad_footprint(c):
    _run_case(c)


@pytest.mark.parametrize("c", T.by_family("elementwise"), ids=_ids(T.by_family("elementwise")))
def test_elementwise_footprint(c):
    _run_case(c)


@pytest.mark.parametrize("c", T.by_family("dense"), ids=_ids(T.by_family("dense")))
def test_dense_wgrad_footprint(c):
    _run_case(c)


# ------------------------------------------------------------------------------------------------------------------ reduce_slots_multi
@pytest.mark.parametrize("n_items", [1, 12])
@pytest.mark.parametrize("weak", [False, True], ids=["natural", "weak-aligned"])
def test_reduce_slots_multi_item_counts(n_items, weak):
    """one launch with 1 item and one with 12 (the maximum), out_t 0 and > 0 side by side, each output in its own guard bands"""
    nat, ops = _ops()
    lib = nat.lib()
    c = next(c for c in T.cases() if c.id == "pw_part_bf16_32x64_ab_db")
    b, p = T.build(c), dict(c.p)
    N, rows, ci, co = p["N"], p["rows"], p["c_in"], p["c_out"]
    A = Arena(weak)
    x, dy, ab = A.operand("x", b.inputs["x"]), A.operand("dy", b.inputs["dy"]), A.operand("ab", b.inputs["ab"])
    ws = A.output("workspace", (lib.pytc_pw_wgrad_slots(N * rows) * (ci * co + co),), F32)
    used = C.c_int(-1)
    _ok(lib.pytc_pw_wgrad_partial(P(x), P(ab), P(dy), P(ws), 1, N, rows, ci, co, nat.BF16, nat.ACT_NONE, C.byref(used), ops._stream()), "partial")
    regs = _check_regions("partial", c, ws, used.value, {})
    part = A.operand("partials", ws[:regs[-1].offset + regs[-1].slots * regs[-1].n].clone())      # an operand now: must not change
    arr = (nat.ReduceItem * n_items)()
    outs = []
    for k in range(n_items):
        r = regs[k % 2]
        out_t = ci if (r.name == "dW" and k % 4 == 0 and n_items > 1) else 0
        o = A.output(f"out{k}", (r.n,), F32)
        arr[k].part, arr[k].out, arr[k].n, arr[k].slots, arr[k].out_t = part[r.offset:].data_ptr(), o.data_ptr(), r.n, r.slots, out_t
        outs.append((r, out_t, o))
    _ok(lib.pytc_reduce_slots_multi(arr, n_items, ops._stream()), f"reduce_slots_multi({n_items})")
    A.check(f"reduce_slots_multi({n_items})")
    seen = set()
    for r, out_t, o in outs:
        assert _sentinels_in(o) == 0
        got = o.view(out_t, r.n // out_t).t().reshape(-1) if out_t else o
        assert torch.equal(got.double(), r.total.to(DEV)), f"item {r.name} out_t {out_t}"
        seen.add(out_t > 0)
    assert seen == ({False} if n_items == 1 else {False, True})


def test_reduce_slots_multi_refuses_a_thirteenth_item():
    nat, ops = _ops()
    A = Arena(False)
    part, out = A.operand("part", torch.ones(2 * 16)), A.output("out", (16,), F32)
    arr = (nat.ReduceItem * 13)()
    for k in range(13):
        arr[k].part, arr[k].out, arr[k].n, arr[k].slots, arr[k].out_t = part.data_ptr(), out.data_ptr(), 16, 2, 0
    st = nat.lib().pytc_reduce_slots_multi(arr, 13, ops._stream())
    torch.cuda.synchronize()
    assert st != nat.OK
    A.check("13 items")
    assert _all_sentinel(out)


def test_pw_wgrad_dgrad_refused_by_its_knob_writes_nothing():
    """wgrad_dgrad_fused = 0: the entry reports unsupported (the caller takes pytc_pw_wgrad(x_act = GELU) + the data-gradient GEMM) and
    leaves every buffer as it was"""
    nat, ops = _ops()
    lib = nat.lib()
    c = next(c for c in T.cases() if c.id == "pw_dgrad_64x32_db")
    b, p = T.build(c), dict(c.p)
    N, rows, ci, co = p["N"], p["rows"], p["c_in"], p["c_out"]
    A = Arena(False)
    x, dy = A.operand("x", b.inputs["x"]), A.operand("dy", b.inputs["dy"])
    wt = A.operand("w_t_paired", ops.pw_pack_weight_paired(b.inputs["w"].to(DEV), transposed=True))
    dx = A.output("dx", (N, rows, ci), BF16)
    ws = A.output("workspace", (lib.pytc_pw_wgrad_slots(N * rows) * (ci * co + co),), F32)
    used = C.c_int(-1)
    with _knobs((("wgrad_dgrad_fused", 0),)):
        assert lib.pytc_pw_wgrad_dgrad_supported(ci, co, nat.BF16) == 0
        st = lib.pytc_pw_wgrad_dgrad_partial(P(x), P(dy), P(wt), P(dx), P(ws), 1, N, rows, ci, co, nat.BF16, C.byref(used), ops._stream())
        torch.cuda.synchronize()
    assert st != nat.OK and used.value == -1
    A.check("refused")
    assert _all_sentinel(dx) and _all_sentinel(ws)
    assert lib.pytc_pw_wgrad_dgrad_supported(ci, co, nat.BF16) == 1


def test_case_count():
    """the table this module runs (recorded in profiles/train_footprint_probe.txt)"""
    n = len(T.cases())
    launches = sum(2 * (1 + len(c.forms)) for c in T.cases())
    print(f"[train_footprint] {n} cases, {launches} guarded runs (forms x alignments), entries: {', '.join(T.table_entries())}")
    assert n == sum(len(T.by_family(f)) for f in T.FAMILIES)

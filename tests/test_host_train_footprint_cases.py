"""CPU checks of the footprint case table (tests/train_footprint_cases.py): the table reaches every edge it claims (by the slot-count
mirrors), the exactness caps hold for every case, one case per family agrees with fp64 torch autograd of the plain operation, the
documented workspace regions tile the queried size without overlap, and every `extern "C"` entry of csrc/train_kernels.hip and of the
four dense weight-gradient launches is either in the table or exempt with a reason."""
import re
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import exact_reduction_cases as X  # noqa: E402
import train_footprint_cases as T  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "pytorch_connectomics_amd" / "csrc"


def _ids(cs):
    return [c.id for c in cs]


# ------------------------------------------------------------------------------------------------------------------ the edges
@pytest.mark.parametrize("c", [c for c in T.cases() if c.family in ("pw", "mixer", "norm")], ids=lambda c: c.id)
def test_claimed_slot_edges_hold_by_the_mirrors(c):
    f = T.slot_facts(c)
    e = set(c.edges)
    if "slots>1" in e:
        assert f["slots"] > 1, f
    if "ragged" in e:
        assert f["ragged"], f
    if "rows%32" in e:
        assert c["rows"] % 32 != 0
    if "straddle" in e:
        assert f["straddle"] and f["block32_straddle"], f
    if "empty_last" in e:
        assert f["empty"] >= 1, f
    if "cap1024" in e:
        assert f["per_split"] == 1024, f
    if "sps>1" in e:
        assert f["per_split"] > 1, f
    if "sps==1" in e:
        assert f["per_split"] == 1, f
    if "mfma" in e:
        assert c["dtype"] == T.BF16 and c["c_in"] % 16 == 0 and c["c_out"] % 16 == 0
    if "valu" in e:
        assert c["dtype"] == T.F32 or c["c_in"] % 16 or c["c_out"] % 16
    if "thin" in e:
        assert 1 in (c["c_in"], c["c_out"]) and not c["ab"] and not c["gelu"]


def test_the_empty_slot_numbers_of_the_issue():
    """66 049 = 257^2 rows: 258 slots of 257 rows, the last one without a row -- generic and matrix-core (32 / 64 channels) alike"""
    assert X.pw_wgrad_slots(T.EMPTY_ROWS) == 258
    assert X.pw_launch_slots(T.EMPTY_ROWS, 32, 64) == 258 and X.pw_launch_slots(T.EMPTY_ROWS, 64, 32) == 258
    assert -(-T.EMPTY_ROWS // 258) == 257 and 257 * 257 == T.EMPTY_ROWS
    assert X.pw_wgrad_slots(T.CAP_ROWS) == 1024 and X.colstats_slots(T.CAP_ROWS) == 1024


@pytest.mark.parametrize("fam", ["pw", "mixer", "norm"])
def test_every_row_slot_family_reaches_every_edge(fam):
    have = set().union(*(set(c.edges) for c in T.by_family(fam)))
    need = {"slots>1", "ragged", "rows%32", "empty_last"}
    if fam == "pw":
        need |= {"straddle", "cap1024", "mfma", "valu", "thin"}
    if fam == "mixer":
        need |= {"sps>1", "sps==1"}
    if fam == "norm":
        need |= {"cap1024"}
    assert need <= have, need - have


def test_depthwise_cases_reach_every_form_and_role():
    forms = set()
    for c in T.by_family("dw"):
        forms.add(T.dw_form(c))
        for kn in c.forms:
            forms.add(T.dw_form(c, kn))
        for tag in ("march", "vec", "generic"):
            if tag in c.edges:
                assert T.dw_form(c) == tag, c.id
        s = T.launch_slots(c)
        assert s is None or s > 1, c.id
        if "ragged" in c.edges:
            vg = c["gdims"][0] * c["gdims"][1] * c["gdims"][2]
            assert vg % 32 != 0
    assert forms == {"march", "vec", "generic"}
    have = set().union(*(set(c.edges) for c in T.by_family("dw")))
    assert "transposed" in have
    assert any(c["K"] == 5 and c["stride"] == 2 for c in T.by_family("dw"))


def test_families_cover_the_forms_the_issue_names():
    pw = T.by_family("pw")
    for entry in ("pytc_pw_wgrad", "pytc_pw_wgrad_partial"):
        cs = [c for c in pw if c.entry == entry]
        for key, vals in (("dtype", {T.BF16, T.F32}), ("ab", {0, 1}), ("gelu", {0, 1}), ("want_db", {0, 1})):
            assert {c[key] for c in cs} == vals, (entry, key)
        assert {(24, 40), (40, 24)} <= {(c["c_in"], c["c_out"]) for c in cs}
        assert any(dict(f).get("wgrad_valu") for c in cs for f in c.forms)
    assert {c["c_in"] for c in pw if c.entry == "pytc_pw_wgrad_dgrad_partial"} == {32, 64, 128}
    mx = [c for c in T.by_family("mixer") if c.entry == "pytc_mixer_bwd_rc"]
    assert {c["c_hid"] for c in mx} == {32, 64, 96} and {c["gn"] for c in mx} == {0, 1} and {c["want_db3"] for c in mx} == {0, 1}
    ap = [c for c in T.by_family("norm") if c.entry == "pytc_norm_bwd_apply"]
    assert {c["s_parts"] for c in ap} == {1, 3} and {c["crop"] for c in ap} == {0, 1}
    assert {(c["dtype"], c["C"]) for c in T.by_family("norm")} >= {(T.BF16, 12), (T.BF16, 32), (T.F32, 12), (T.F32, 32)}
    for c in T.by_family("elementwise"):
        if "n%vec" in c.edges:
            n = c.get("n") or c["N"] * c["rows"] * c["C"]
            assert n % 8 != 0, c.id
    assert {c.entry for c in T.by_family("dense")} == set(T.DENSE_ENTRIES)
    knobs = {k for c in T.cases() for f in c.forms for k, _ in f} | {"wgrad_dgrad_fused"}      # (the GPU module's refusal case)
    assert knobs <= set(T.KNOB_DEFAULTS)
    assert knobs >= set(T.KNOB_DEFAULTS) - {"elementwise_vec"}      # no launch of these families reads elementwise_vec


# ------------------------------------------------------------------------------------------------------------------ caps and regions
@pytest.mark.parametrize("c", T.cases(), ids=_ids(T.cases()))
def test_caps_hold_and_references_are_storage_numbers(c):
    b = T.build(c)                       # asserts assert_exact_cap / gemm_abs_bound / is_bf16_exact as it builds
    assert b.outputs or b.totals
    for name, r in b.outputs.items():
        assert r.ref.dtype == torch.float64 and bool(torch.isfinite(r.ref).all()), name
        assert r.ulp == 0 or (c.entry == "pytc_norm_bwd" and name == "dt" and r.dtype == T.BF16)
    for name, t in b.inputs.items():
        if isinstance(t, torch.Tensor) and t.is_floating_point():
            assert bool(torch.isfinite(t).all()), name


@pytest.mark.parametrize("c", [c for c in T.cases() if T.regions(c, 2)], ids=lambda c: c.id)
def test_regions_tile_the_workspace_the_queries_promise(c):
    """the documented regions are disjoint, in order, and end inside the size the query's formula gives for the mirrored slot count"""
    for kn in ((),) + c.forms:
        S = T.launch_slots(c, kn)
        if S is None:
            S = 6                                    # no mirror (fp32 depthwise): any count shows the layout
        rs = T.regions(c, S)
        end = 0
        for r in rs:
            assert r.offset == end, (c.id, r.name)
            end = r.offset + r.slots * r.n
            assert r.total is None or r.total.numel() == r.n, (c.id, r.name)
            assert r.written is False or r.total is not None, (c.id, r.name)
        p = dict(c.p)
        if c.family == "pw":
            bound = X.pw_wgrad_slots(p["N"] * p["rows"]) * (p["c_in"] * p["c_out"] + p["c_out"])
        elif c.family == "dw":
            bound = S * (p["K"] ** 3 * p["C"] + p["C"])
        elif c.entry == "pytc_mixer_bwd_rc":
            per = 32 * p["c_hid"]
            bound = S * (per + 32) + (S * (per + p["c_hid"]) + p["N"] * (per + p["c_hid"]) if p["gn"] else 0)
        else:
            per = p["c"] * p["c_hid"] + p["c_hid"]
            bound = S * per + p["N"] * per
        assert end <= bound, (c.id, kn, end, bound)
        if c.family == "mixer":
            assert end == bound


# ------------------------------------------------------------------------------------------------------------------ autograd
def _first(entry, **kv):
    for c in T.cases():
        if c.entry == entry and all(c.get(k) == v for k, v in kv.items()):
            return c
    raise AssertionError(entry)


def _eq(a, b, what):
    assert tuple(a.shape) == tuple(b.shape), what
    assert torch.equal(a.double(), b.double()), f"{what}: max |diff| {float((a.double() - b.double()).abs().max())}"


def test_autograd_pw():
    c = _first("pytc_pw_wgrad_dgrad_partial", c_in=64, want_db=1, N=3)
    b = T.build(c)
    hp = b.inputs["x"].double().requires_grad_()
    W = b.inputs["w"].double().requires_grad_()
    bias = torch.zeros(c["c_out"], dtype=torch.float64, requires_grad=True)
    y = F.gelu(hp) @ W.t() + bias
    (y * b.inputs["dy"].double()).sum().backward()
    _eq(W.grad.reshape(-1), b.totals["dW"], "dW")
    _eq(bias.grad, b.totals["db"], "db")
    _eq(hp.grad, b.outputs["dx"].ref, "dx")
    c = _first("pytc_pw_wgrad", ab=1, dtype=T.BF16, c_in=32)
    b = T.build(c)
    ab = b.inputs["ab"].double()
    xn = b.inputs["x"].double() * ab[:, 0][:, None] + ab[:, 1][:, None]
    W = torch.zeros((c["c_out"], c["c_in"]), dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(c["c_out"], dtype=torch.float64, requires_grad=True)
    ((xn @ W.t() + bias) * b.inputs["dy"].double()).sum().backward()
    _eq(W.grad, b.outputs["dW"].ref, "dW")
    _eq(bias.grad, b.outputs["db"].ref, "db")


def test_autograd_mixer():
    c = _first("pytc_mixer_bwd_rc", c_hid=64, gn=1, want_db3=1, N=2)
    b = T.build(c)
    i = b.inputs
    t = i["t"].double()
    mean, rstd = i["mr"][:, 0].double()[:, None], i["mr"][:, 1].double()[:, None]
    gamma = i["gamma"].double()
    beta = (i["ab"][:, 1].double() + i["mr"][:, 0].double() * i["ab"][:, 0].double())[:, None]
    xhat = (t - mean) * rstd
    xn = (xhat * gamma + beta).requires_grad_()
    W2, W3 = i["w2"].double().requires_grad_(), i["w3"].double().requires_grad_()
    b2 = i["b2"].double().requires_grad_()
    b3 = torch.zeros(32, dtype=torch.float64, requires_grad=True)
    hp = xn @ W2.t() + b2
    hp.retain_grad()
    y = F.gelu(hp) @ W3.t() + b3
    (y * i["dy"].double()).sum().backward()
    _eq(hp.grad, b.outputs["dhp"].ref, "dhp")
    _eq(W3.grad.reshape(-1), b.totals["dW3"], "dW3")
    _eq(b3.grad, b.totals["db3"], "db3")
    _eq(W2.grad.reshape(-1), b.totals["dW2"], "dW2")
    _eq(b2.grad, b.totals["db2"], "db2")
    dtn = xn.grad
    _eq(torch.stack([dtn.sum(1), (dtn * xhat).sum(1)], 1), b.outputs["s_out"].ref, "s_out")
    # coef: dt = A dtn + B t + C is the GroupNorm backward rstd gamma (dtn - S1 / count - xhat S2 / count)
    s, count, coef = b.outputs["s_out"].ref, i["count"], b.outputs["coef"].ref
    want = (rstd * gamma) * (dtn - s[:, 0][:, None] / count - xhat * s[:, 1][:, None] / count)
    got = coef[:, 0][:, None] * dtn + coef[:, 1][:, None] * t + coef[:, 2][:, None]
    _eq(got, want, "coef")


def test_autograd_norm():
    c = _first("pytc_norm_bwd_stats", dtype=T.BF16, C=12)
    b = T.build(c)
    t, mr = b.inputs["t"].double(), b.inputs["mr"].double()
    N, C = c["N"], c["C"]
    g = torch.ones((N, 1, C), dtype=torch.float64, requires_grad=True)         # per-sample scale and shift: their gradients are the sums
    sh = torch.zeros((N, 1, C), dtype=torch.float64, requires_grad=True)
    xhat = (t - mr[:, 0][:, None]) * mr[:, 1][:, None]
    ((xhat * g + sh) * b.inputs["dtn"].double()).sum().backward()
    _eq(torch.stack([sh.grad[:, 0], g.grad[:, 0]], 1), b.outputs["s_out"].ref, "s_out")
    # GroupNorm(C, C) with the data's own statistics: pytc_norm_bwd's formula is autograd's
    x = torch.randn(2, 50, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1)).requires_grad_()
    d = torch.randn(2, 50, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    gam = torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64)
    mean, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
    rstd = (var + 1e-5).rsqrt()
    xh = (x - mean) * rstd
    ((xh * gam) * d).sum().backward()
    dtn = d
    want = rstd * gam * (dtn - dtn.mean(1, keepdim=True) - xh * (dtn * xh).mean(1, keepdim=True))
    assert torch.allclose(x.grad, want.detach(), rtol=0, atol=1e-12)


def test_autograd_dw():
    for c in (_first("pytc_dw_wgrad", K=3, stride=2, want_db=1), _first("pytc_dw_wgrad", K=5, stride=2, want_db=1)):
        b = T.build(c)
        K, C = c["K"], c["C"]
        x = b.inputs["x"].double().permute(0, 4, 1, 2, 3)
        w = torch.zeros((C, 1, K, K, K), dtype=torch.float64, requires_grad=True)
        bias = torch.zeros(C, dtype=torch.float64, requires_grad=True)
        y = F.conv3d(x, w, bias, stride=c["stride"], padding=K // 2, groups=C)
        assert tuple(y.shape[2:]) == tuple(c["gdims"])
        (y * b.inputs["g"].double().permute(0, 4, 1, 2, 3)).sum().backward()
        _eq(w.grad.view(C, K ** 3).t(), b.outputs["dW"].ref, c.id + " dW")
        _eq(bias.grad, b.outputs["db"].ref, c.id + " db")
    c = _first("pytc_dw_wgrad", K=3, stride=2, want_db=0)                      # the transposed conv: g = its input, x = dL/dy
    b = T.build(c)
    C = c["C"]
    w = torch.zeros((C, 1, 3, 3, 3), dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose3d(b.inputs["g"].double().permute(0, 4, 1, 2, 3), w, stride=2, padding=1, groups=C)
    assert tuple(y.shape[2:]) == tuple(c["xdims"])
    (y * b.inputs["x"].double().permute(0, 4, 1, 2, 3)).sum().backward()
    _eq(w.grad.view(C, 27).t(), b.outputs["dW"].ref, c.id + " dW")


def test_autograd_elementwise():
    b = T.build(_first("pytc_gelu", bwd=1, dtype=T.BF16, n=1003))
    x = b.inputs["x"].double().requires_grad_()
    (F.gelu(x) * b.inputs["dy"].double()).sum().backward()
    _eq(x.grad, b.outputs["out"].ref, "gelu'")
    b = T.build(_first("pytc_grn_bwd_apply", dtype=T.BF16))
    hp = b.inputs["hp"].double().requires_grad_()
    A, B = b.inputs["A"].double()[:, None], b.inputs["B"].double()[:, None]
    h = F.gelu(hp)
    # out = dL/dhp of L = sum(dh2 (h A)) + sum(B h^2 / 2): (dh2 A + h B) gelu'(hp)
    ((b.inputs["dh2"].double() * h * A).sum() + (B * h * h / 2).sum()).backward()
    _eq(hp.grad, b.outputs["out"].ref, "grn_bwd_apply")


def test_autograd_dense():
    c = _first("pytc_conv3d_wgrad", dtype=T.BF16, k=(3, 3, 3))
    b = T.build(c)
    co, ci, k = c["c_out"], c["c_in"], c["k"]
    w = torch.zeros((co, ci, *k), dtype=torch.float64, requires_grad=True)
    y = F.conv3d(b.inputs["a"].double().permute(0, 4, 1, 2, 3), w, padding=tuple(v // 2 for v in k))
    (y * b.inputs["dy"].double().permute(0, 4, 1, 2, 3)).sum().backward()
    _eq(w.grad.permute(2, 3, 4, 0, 1).reshape(-1, co, ci), b.outputs["dW"].ref, "conv3d dW")
    c = _first("pytc_conv3d_wgrad_strided", dtype=T.BF16)
    b = T.build(c)
    w = torch.zeros((c["c_o"], c["c_k"], 3, 3, 3), dtype=torch.float64, requires_grad=True)
    y = F.conv3d(b.inputs["big"].double().permute(0, 4, 1, 2, 3), w, stride=2, padding=1)
    (y * b.inputs["small"].double().permute(0, 4, 1, 2, 3)).sum().backward()
    _eq(w.grad.permute(2, 3, 4, 0, 1).reshape(27, c["c_o"], c["c_k"]), b.outputs["dW"].ref, "strided dW")
    for entry in ("pytc_upcat_deconv2_wgrad", "pytc_deconv2_upfirst_wgrad"):
        c = _first(entry, dtype=T.BF16, N=2)
        b = T.build(c)
        ci, cu, ce, lo = c["c_in"], c["c_u"], c["c_e"], c["lo"]
        w = torch.zeros((ci, cu, 2, 2, 2), dtype=torch.float64, requires_grad=True)
        bias = torch.zeros(cu, dtype=torch.float64, requires_grad=True)
        up = F.conv_transpose3d(b.inputs["x_low"].double().permute(0, 4, 1, 2, 3), w, bias, stride=2)
        d = b.inputs["d"].double().permute(0, 4, 1, 2, 3)
        if entry == "pytc_upcat_deconv2_wgrad":
            sk = c["sk"]
            up = F.pad(up, (0, sk[2] - 2 * lo[2], 0, sk[1] - 2 * lo[1], 0, sk[0] - 2 * lo[0]), mode="replicate")
            (up * d[:, ce:]).sum().backward()
        else:
            (up * d[:, :cu]).sum().backward()
        _eq(w.grad, b.outputs["dw"].ref, entry + " dw")
        _eq(bias.grad, b.outputs["db"].ref, entry + " db")


# ------------------------------------------------------------------------------------------------------------------ completeness
def _entries(path, names=None):
    text = (CSRC / path).read_text()
    found = re.findall(r'^extern "C" (?:int|int64_t) (pytc_\w+)\s*\(', text, flags=re.M)
    return [n for n in found if names is None or n in names]


def test_every_train_entry_has_a_case_or_an_exemption():
    train = _entries("train_kernels.hip")
    assert len(train) >= 25 and "pytc_mixer_bwd_rc" in train and "pytc_mixer_bwd_rc_ws_elems" in train
    dense = (_entries("rsunet_train_kernels.hip", T.DENSE_ENTRIES) + _entries("conv3d_strided_kernels.hip", T.DENSE_ENTRIES) +
             _entries("upcat_kernels.hip", T.DENSE_ENTRIES))
    assert sorted(dense) == sorted(T.DENSE_ENTRIES)
    table = set(T.table_entries())
    missing = [n for n in train + dense if n not in table and n not in T.EXEMPT]
    assert not missing, f"entries without a footprint case or an EXEMPT reason: {missing}"
    both = [n for n in table if n in T.EXEMPT and n != T.REDUCE_ENTRY]
    assert not both, f"entries that are exempt AND in the table: {both}"
    header = (ROOT / "include" / "pytc_hip.h").read_text()
    stale = [n for n in list(T.EXEMPT) + sorted(table) if not re.search(rf"\b{n}\(", header)]
    assert not stale, f"names that are no entry of the C ABI any more: {stale}"
    assert all(len(r) > 8 for r in T.EXEMPT.values())


def test_exempt_queries_are_exactly_the_query_suffixes():
    for n, reason in T.EXEMPT.items():
        if reason.startswith("host query"):
            assert re.search(r"_(supported|slots|sps|ws_elems)$", n), n


def test_knob_defaults_are_the_library_table():
    """KNOB_DEFAULTS is what the GPU module restores after every form: it must be the X(name, default, ...) table of pytc_common.h"""
    rows = dict(re.findall(r"^\s*X\((\w+), ([^,]+),", (CSRC / "pytc_common.h").read_text(), flags=re.M))
    assert len(rows) >= 20
    for k, v in T.KNOB_DEFAULTS.items():
        assert k in rows and int(eval(rows[k], {"__builtins__": {}})) == v, (k, rows.get(k), v)

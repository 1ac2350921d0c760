"""Host proof for tests/test_gpu_mixer_exact.py (no GPU): the bit model of the packed-fp16 GELU reproduces what the comment next to
gelu_h2 claims and has the special values no other test pins; every filed case meets its exactness premises and discriminates
(mixer_exact_cases.assert_premises); a restatement of every kernel form in fp32 numpy -- the model in the middle -- passes the
assertion the GPU test makes; and each of sixteen seeded defects fails at least one filed case."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import mixer_exact_cases as X  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pytorch_connectomics_amd" / "csrc"


# ------------------------------------------------------------------------------------------------------------- the model
def test_model_coefficients_are_the_kernels():
    src = (CSRC / "pytc_common.h").read_text()
    body = src[src.index("h8_t gelu_h8_from_f32"):src.index("Bijective XCD-aware remap")]
    lits = [float(v) for v in re.findall(r"(-?\d\.\d+e-\d\d)f\)", body)]
    assert tuple(lits) == X.GELU_COEFFS
    assert "PYTC_H2C(3.75f)" in body and "PYTC_H2C(2.0f / 3.75f)" in body and "PYTC_H2C(-1.0f)" in body and "cvt_pkrtz" in body
    plain = src[src.index("h2_t gelu_h2(h2_t x)"):src.index("eight fp32 pre-activations")]
    assert tuple(float(v) for v in re.findall(r"(-?\d\.\d+e-\d\d)f\)", plain)) == X.GELU_COEFFS


def test_model_accuracy_is_what_the_source_comment_claims():
    """over every f16 input in [-8, 8]: max |error| against the fp64 erf GELU, where it lies, and the mean -- to the two digits the
    comment gives"""
    x = X.all_f16_in(-8.0, 8.0)
    assert len(x) == 36866
    err = np.abs(X.gelu_h8_model(x.astype(np.float32)).astype(np.float64) - X.erf_gelu64(x.astype(np.float64)))
    at = float(abs(x[int(err.argmax())]))
    src = (CSRC / "pytc_common.h").read_text()
    m = re.search(r"max \|error\| ([0-9.e-]+) at \|x\| ~ ([0-9.]+) .*?mean ([0-9.e-]+)\.", src, re.S)
    assert m, "the accuracy claim next to gelu_h2 is gone"
    assert f"{err.max():.1e}" == f"{float(m.group(1)):.1e}" == "1.1e-03"
    assert f"{err.mean():.1e}" == f"{float(m.group(3)):.1e}" == "1.5e-04"
    assert f"{at:.1f}" == m.group(2) == "3.5", (at, m.group(2))
    assert at == 3.490234375 and abs(err.max() - 1.111e-3) < 5e-7 and abs(err.mean() - 1.49e-4) < 5e-7


def test_model_special_values():
    g = X.gelu_h8_model(np.float32([0.0, -0.0]))
    assert (g.view(np.uint16) == np.float16(2.0 ** -14).view(np.uint16)).all()              # gelu_h2(+-0) = 2^-14, not 0
    tail = np.concatenate([X.all_f16_in(-65504.0, -3.75).astype(np.float32), np.float32([-65520.0, -1e5, -3e38, -3.7500002])])
    gt = X.gelu_h8_model(tail)
    assert len(set(gt.view(np.uint16).tolist())) == 1 and float(gt[0]) == float(np.float16(-1.498e-4))     # the saturated negative tail
    top = X.gelu_h8_model(np.float32([65504.0, 65519.9, 65520.0, 1e5, 3e38]))
    assert len(set(top.view(np.uint16).tolist())) == 1 and float(top[0]) == 65504.0          # saturating conversion: finite in, finite out
    sub = X.f32_to_f16_rtz(np.float32([2.0 ** -25, -2.0 ** -25, 2.0 ** -24 * 1.75, 6.0e-5]))
    assert sub.tolist() == [0.0, -0.0, 2.0 ** -24, 2.0 ** -24 * 1006]                        # toward zero into the subnormals


def test_conversion_modes_differ_on_the_conversion_inputs():
    for c in X.cases("conv"):
        h = X.reference(c)["h"].astype(np.float32)
        rtz, rne = X.f32_to_f16_rtz(h), X.f32_to_f16_rne(h)
        n = int((rtz.view(np.uint16) != rne.view(np.uint16)).sum())
        assert n >= h.size // 4, (c.id, n, h.size)                                           # the dropped bits are past the midpoint about half the time
        ng = int((X.gelu_h8_model(h).view(np.uint16) != X.gelu_h8_model(h, rne=True).view(np.uint16)).sum())
        assert ng >= h.size // 8, (c.id, ng)
    mids = X.sweep_inputs()["midpoints"]
    assert int((X.f32_to_f16_rtz(mids).view(np.uint16) != X.f32_to_f16_rne(mids).view(np.uint16)).sum()) >= len(mids) // 3


def test_an_unfused_t_differs():
    """t = round(round(u c) - 1) instead of one FMA: 2704 of the 36866 f16 inputs in [-8, 8] give other bits"""
    x = X.sweep_inputs()["f16 in [-8, 8]"]
    n = int((X.gelu_h8_model(x).view(np.uint16) != X.gelu_h8_model(x, unfused_t=True).view(np.uint16)).sum())
    assert n == UNFUSED_T_DIFFERS, n


UNFUSED_T_DIFFERS = 2704


def test_sweep_inputs_cover_what_the_gpu_sweep_claims():
    s = X.sweep_inputs()
    assert len(s["f16 in [-8, 8]"]) == 36866 and 200 <= len(s["large"]) <= 400
    big = s["large"].astype(np.float64)
    assert (np.abs(big) > 8).all() and (np.abs(big) > 65504).sum() >= 6 and (np.abs(big) == 65504).sum() == 2
    m = s["midpoints"]
    assert (X.f32_to_f16_rne(m).astype(np.float32) != m).all()                               # none is an f16 number
    sub = s["subnormal images"]
    img = X.f32_to_f16_rtz(sub).astype(np.float64)
    assert (np.abs(img) < 2.0 ** -14).all() and (np.abs(sub) >= 2.0 ** -126).all()           # subnormal f16 images of NORMAL fp32 inputs
    assert (img == 0).sum() >= 3 and (img != 0).sum() >= 100


# ------------------------------------------------------------------------------------------------------------- the cases
def test_the_filed_cases_cover_what_the_gpu_suite_claims():
    st = X.cases("stream")
    per = {}
    for c in st:
        per.setdefault((c.cin // 32, c.cout // 16), []).append(c)
    assert set(per) == set(X.MLP_INSTANCES)
    src = (CSRC / "pw_mlp_kernels.hip").read_text()
    assert {(int(a), int(b)): int(n) for a, b, n in re.findall(r"PYTC_MLP_CASE\((\d+), (\d+), (\d+)\)", src)} == X.MLP_INSTANCES
    for (ks, mo), cs in per.items():
        nt = X.MLP_INSTANCES[(ks, mo)]
        wg = 4 * nt * 16
        plain = [c for c in cs if not c.n_head and c.res != "stem"]
        assert {(c.form, c.res) for c in plain} >= {(f, r) for f in ("affine", "folded") for r in ("none", "add", "up", "up_low")}
        assert {c.chid for c in plain} >= {32, 64, 96, X.widest_hidden(ks, mo)}
        rows = {c.rows for c in plain}
        assert 1 in rows and wg in rows and wg + 1 in rows and wg + nt * 16 + 3 in rows, (ks, mo, rows)
        assert {c.N for c in plain} == {1, 3} and {c.family for c in plain} == {"sparse", "dense"}
        # both sides of PREFETCH_RES ((MO / 2) * NT <= 4) occur over the instances, each with a residual
    assert {(mo // 2) * nt <= 4 for (ks, mo), nt in X.MLP_INSTANCES.items()} == {True, False}
    assert X.widest_hidden(8, 8) == 2048 and sum(X.widest_hidden(*k) == 1024 for k in X.MLP_INSTANCES) >= 1
    assert any(c.grid == (4, 4, 6) for c in st)                                              # 16-row tiles straddle y and z carries
    dma = X.cases("dma")
    assert {c.rows for c in dma} == {1, 63, 577} and {c.chid for c in dma} == {64, 96, 128}
    assert {dict(c.knobs)["mlp_dma_wgs"] for c in dma} == {0, 1, 3} and {dict(c.knobs)["mlp_dma"] for c in dma} == {0, 1}
    assert {c.n_head for c in dma} == {0, 1, 3, 16} and {c.head_bias for c in dma if c.n_head} == {True, False}
    assert {(c.cin, c.cout) for c in X.cases("lds")} == set(X.LDS_FAMILIES) and {(c.cin, c.cout) for c in X.cases("chunk")} == set(X.CHUNK_FAMILIES)
    assert {dict(c.knobs)["pw_gemm_rows"] for c in X.cases("gemm")} == {0, 64, 128}
    assert {c.res for c in X.cases("gemm")} == {"none", "add", "up", "up_low"}
    hdr = (CSRC / "pytc_common.h").read_text()
    for k, v in X.KNOB_DEFAULTS.items():
        m = re.search(r"X\(%s, ([^,]+)," % k, hdr)
        assert m and eval(m.group(1)) == v, k


GROUPS = ["stream", "dma", "lds", "chunk", "gemm", "conv", "dwmix"]


@pytest.mark.parametrize("group", GROUPS)
def test_every_filed_case_meets_its_premises(group):
    for c in X.cases(group):
        X.assert_premises(c)
        if c.conv and c.form == "affine":
            X.assert_premises(c, True)


def test_larger_expand_weights_would_break_the_premise():
    """why |h| <= 2.75: with pre-activations below -3.75 the hidden sits in the saturated tail, whose unit is 2^-23"""
    g = float(X.gelu_h8_model(np.float32([-4.75]))[0])
    assert g * 2.0 ** 16 != round(g * 2.0 ** 16)
    with pytest.raises(AssertionError):
        X.exact_sum(np.array([[g * 0.5, 34.0]]), "tail")


# ------------------------------------------------------------------------------------------------------------- restatement
DEFECTS = ("drop_last_chunk", "swap_chunks", "paired_row", "rne", "hidden_bf16", "unfused_t", "b3_twice", "truncate", "round_twice",
           "sample0_operands", "clamped_row_stored", "res_low_shift", "no_res_bias", "face_mixer", "storeh_unrounded", "head_unrounded")


def _f32(v):
    return np.asarray(v, dtype=np.float32)


def _rb(v32):
    """fp32 -> bf16 -> fp32, round to nearest even"""
    return torch.from_numpy(np.ascontiguousarray(v32, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def _tb(v32):
    b = np.ascontiguousarray(v32, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return b.view(np.float32)


def restate(c, defect=None, train=False):
    """every kernel form in fp32 numpy, in the kernels' order of operations: affine in fp32 -> bf16 operand, GEMM1 from the bias,
    (training: bf16 store of the pre-activation, GELU at the stored value), the model, GEMM2 from b3 over the hidden chunks, the
    epilogue, ONE store.  -> dict of torch tensors named as the GPU test names them, plus "guard": rows stored past the tensor."""
    d = X.operands(c)
    N, R = c.N, c.rows
    t = _f32(d["t"])
    if c.dims:                                       # the fused block forms t itself: depthwise conv in fp32, stored as bf16
        cin = c.cin
        xt = torch.from_numpy(_f32(d["x5"])).permute(0, 4, 1, 2, 3)
        wt = torch.from_numpy(_f32(d["taps"]).T.reshape(cin, 1, 3, 3, 3).copy())
        conv = torch.nn.functional.conv3d(xt, wt, torch.from_numpy(_f32(d["dw_bias"])), padding=1, groups=cin)
        t = conv.permute(0, 2, 3, 4, 1).reshape(N, R, cin).to(torch.bfloat16).float().numpy()
    pick = (lambda n: 0) if defect == "sample0_operands" else (lambda n: n)
    if d["ab"] is not None:
        ab = _f32(d["ab"])
        xe = np.stack([_rb(t[n] * ab[pick(n), 0][None] + ab[pick(n), 1][None]) for n in range(N)])
        w2 = np.broadcast_to(_f32(d["w2"]), (N, c.chid, c.cin))
        b2 = np.broadcast_to(_f32(d["b2"]), (N, c.chid))
    else:
        xe = t
        w2 = np.stack([_f32(d["w2"])[pick(n)] for n in range(N)])
        b2 = np.stack([_f32(d["b2"])[pick(n)] for n in range(N)])
    if defect == "paired_row":                       # the image built with the (T & 1) * 4 term lost: rows with bit 2 set never loaded
        j = np.arange(c.chid)
        w2 = w2[:, j & ~4]
    h = np.einsum("nrk,njk->nrj", xe, w2).astype(np.float32) + b2[:, None, :]
    out = {}
    hin = h
    if train:
        out["hidden_pre"] = torch.from_numpy(h).to(torch.bfloat16)
        if defect != "storeh_unrounded":
            hin = out["hidden_pre"].float().numpy()
    g = X.gelu_h8_model(hin, rne=defect == "rne", unfused_t=defect == "unfused_t").astype(np.float32)
    if defect == "hidden_bf16":
        g = _rb(g)
    out["g"] = torch.from_numpy(g.astype(np.float16))
    w3 = _f32(d["w3"]).copy()
    HC = c.chid // 32
    if defect == "drop_last_chunk":
        w3[:, -32:] = 0
    if defect == "swap_chunks":
        w3 = w3.reshape(c.cout, HC, 32)[:, ::-1].reshape(c.cout, c.chid)
    b3 = _f32(d["b3"])
    acc = b3[None, None] + g @ w3.T
    if defect == "b3_twice":
        acc = acc + b3[None, None]
    store = _tb if defect == "truncate" else _rb
    unrounded = acc
    if c.res == "add":
        res = _f32(d["res"])
        unrounded = acc + res
        y = store(_rb(acc) + res) if defect == "round_twice" else store(acc + res)
    elif c.res == "stem":
        res = _rb(_f32(d["stem_w"])[None, None] * _f32(d["x0"])[:, :, None] + _f32(d["stem_b"])[None, None])
        unrounded = acc + res
        y = store(_rb(acc) + res) if defect == "round_twice" else store(acc + res)
    elif c.res in ("up", "up_low"):
        face, even, low = X.upsample_parts(c)
        sk = _f32(d["res"])
        rl = np.broadcast_to(_f32(d["res_bias"]), acc.shape).copy()
        if defect == "no_res_bias":
            rl[:] = 0
        if c.res == "up_low":
            if defect == "res_low_shift":
                # res_low taken at (o + 1) >> 1, o = position - 1: at an even o that is the SAME element, so the seeded defect is the
                # one that moves an element -- parity test and index both on o + 1 (positions even in every axis take res_low)
                D, H, W = c.grid
                z, yy, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
                even = (~face.reshape(D, H, W) & (((z | yy | x) & 1) == 0)).reshape(-1)
                low = (((z >> 1) * (H // 2) + (yy >> 1)) * (W // 2) + (x >> 1)).reshape(-1)
            rl[:, even] = _f32(d["res_low"])[:, low[even]]
        full = store(_rb(acc) + rl + sk) if defect == "round_twice" else store(acc + rl + sk)
        y = full if defect == "face_mixer" else np.where(face[None, :, None], sk, full)
    else:
        y = store(acc)
    # the launch writes sample after sample; "clamped_row_stored": the rows of the last tile past rps hold the clamped row rps - 1 and
    # are stored too -- into the next sample's first rows (overwritten when that sample is written) or past the tensor
    nt = X.MLP_INSTANCES.get((c.cin // 32, c.cout // 16), 2)
    pad = (-R) % (nt * 16)
    flat = np.full((N * R + pad, c.cout), np.nan, np.float32)
    for n in range(N):
        flat[n * R:(n + 1) * R] = y[n]
        if defect == "clamped_row_stored" and pad:
            flat[(n + 1) * R:(n + 1) * R + pad] = y[n, R - 1]
    out["guard"] = flat[N * R:]
    yv = flat[:N * R].reshape(N, R, c.cout)
    out["y"] = torch.from_numpy(yv.copy()).to(torch.bfloat16)
    yin = unrounded if defect == "head_unrounded" else yv
    if c.n_head:
        hb = _f32(d["head_b"]) if d["head_b"] is not None else np.zeros(c.n_head, np.float32)
        out["logits"] = torch.from_numpy((yin @ _f32(d["head_w"]).T + hb[None, None]).astype(np.float32))
    if c.proj:
        out["z"] = torch.from_numpy(yin @ _f32(d["proj_w"]).T + _f32(d["proj_b"])[None, None]).to(torch.bfloat16)
    return out


def passes(c, out, train=False) -> bool:
    """the GPU test's assertion: every output the case has carries the reference's bits, and nothing was stored past the tensor"""
    ref = X.reference(c, train)
    keys = ["y"] + (["logits"] if c.n_head else []) + (["z"] if c.proj else []) + (["hidden_pre"] if train else [])
    if c.group == "gemm":
        keys.append("g")
    for k in keys:
        want = torch.from_numpy(ref[k].copy()) if k == "g" else ref[k]
        try:
            X.check_bits(out[k], want, f"{c.id}: {k}")
        except AssertionError:
            return False
    return bool(np.isnan(out["guard"]).all())


@pytest.mark.parametrize("group", GROUPS)
def test_the_restatement_passes_every_case(group):
    seen = set()
    for c in X.cases(group):
        if c.data_key in seen:
            continue
        seen.add(c.data_key)
        assert passes(c, restate(c)), c.id
        if c.conv and c.form == "affine":
            assert passes(c, restate(c, train=True), True), c.id


def _defect_cases():
    """a small filed subset with every form in it: ragged rows, several chunks, N = 3, both up-sampling forms, stem, head, projection,
    the GEMM pair (whose hidden is compared as well) and the conversion cases"""
    st = X.cases("stream")
    pick = [c for c in st if c.cin <= 64 and c.chid <= 128][:16]
    pick += [c for c in st if c.n_head or c.res == "stem"]
    pick += [c for c in X.cases("dma") if dict(c.knobs)["mlp_dma_wgs"] == 1 and c.rows == 63]
    pick += X.cases("gemm")[:4] + X.cases("conv") + X.cases("dwmix")[:1] + X.cases("dwmix")[4:5]
    return pick


@pytest.mark.parametrize("defect", DEFECTS)
def test_every_seeded_defect_fails_a_filed_case(defect):
    red = []
    for c in _defect_cases():
        if defect == "storeh_unrounded":
            if c.conv and c.form == "affine" and not passes(c, restate(c, defect, True), True):
                red.append(c.id)
            continue
        if not passes(c, restate(c, defect)):
            red.append(c.id)
    assert red, f"{defect}: no filed case notices"
    print(f"{defect}: {len(red)} cases red, e.g. {red[:3]}")

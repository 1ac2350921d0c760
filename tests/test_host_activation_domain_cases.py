"""Host proofs for tests/activation_domain_cases.py (no GPU): the claims the source comments of csrc/pytc_common.h make about the GELU
forms, measured in fp64 over every bf16 value and the fp32 grid; the forward / backward pairing table of the training schedules; that
every seeded change to a model leaves the real model's interval for some input of the sweep (so the GPU cases can see it); the class
rules; and, per row of the entry-point table, that the operands around the activation make the surrounding GEMM exact."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import activation_domain_cases as X  # noqa: E402

D = np.float64


def _finite_bf16():
    b = X.bf16_all().ravel()
    return b[np.isfinite(b)]


SWEEPS = {"bf16_all": _finite_bf16, "f32_grid": lambda: X.f32_grid().ravel()}


def _three_figures(measured: float, claim: float, what: str):
    """measured <= claim, and claim is the measured value to three significant figures (rounded up): nothing looser is written down"""
    print(f"{what}: measured {measured:.6e}, claim {claim:.3e}")
    assert measured <= claim, f"{what}: {measured:.6e} > {claim:.3e}"
    assert measured >= claim * (1.0 - 1.0e-2), f"{what}: the claim {claim:.3e} is looser than three figures of the measured {measured:.6e}"


# ------------------------------------------------------------------------------------------------------------ inputs
def test_inputs_are_what_the_module_says():
    b = X.bf16_all()
    assert b.shape == (2048, 32) and b.dtype == np.float32
    bits = (b.ravel().view(np.uint32) >> 16)
    assert np.array_equal(bits, np.arange(65536)) and not (b.ravel().view(np.uint32) & 0xFFFF).any()
    assert int(np.isfinite(b).sum()) == 65280 and int(np.isnan(b).sum()) == 254 and int(np.isinf(b).sum()) == 2
    g = X.f32_grid()
    assert g.shape == X.GRID_SHAPE and g.size == 1 << 19 and np.isfinite(g).all()
    have = set(g.ravel().view(np.uint32).tolist())
    fin = _finite_bf16()
    for v in (fin, np.nextafter(fin, np.float32(np.inf)), np.nextafter(fin, np.float32(-np.inf))):
        v = v[np.isfinite(v)]
        assert set(v.view(np.uint32).tolist()) <= have
    eight = np.float32(8.0)
    for v in (3.75, -3.75, 8.0, -8.0, np.nextafter(eight, np.float32(0)), np.nextafter(eight, np.float32(9))):
        assert int(np.float32(v).view(np.uint32)) in have
    # the round trip the GPU tests rely on
    t = X.to_bf16_tensor(b)
    assert np.array_equal(X.from_bf16_tensor(t).view(np.uint32), b.view(np.uint32))
    # round_bf16 is round-to-nearest-even and the identity on bf16 numbers
    assert np.array_equal(X.round_bf16(fin).view(np.uint32), fin.view(np.uint32))
    import torch
    r = np.random.default_rng(0).standard_normal(4096).astype(np.float32) * 7
    assert np.array_equal(X.round_bf16(r), torch.from_numpy(r).to(torch.bfloat16).float().numpy())


# ------------------------------------------------------------------------------------------------------------ claims of the comments
@pytest.mark.parametrize("sweep", list(SWEEPS))
def test_claims_of_the_source_comments(sweep):
    x = SWEEPS[sweep]().astype(D)
    z = x * np.sqrt(0.5)
    as_err = np.abs(X._as_one_plus_erf64(z) - (1.0 + X._erf64(z)))
    _three_figures(as_err.max(), 1.40e-7, "A&S 7.1.26 1 + erf, abs error")
    assert as_err.max() <= 1.5e-7                                           # what pytc_common.h says
    ge = np.abs(X.gelu_erf64(x) - X.gelu64(x))
    _three_figures(ge.max(), 2.12e-7, "gelu_erf abs error")
    assert (ge <= 0.5 * np.abs(x) * as_err.max() * (1 + 1e-12) + 1e-300).all(), "gelu_erf error is not bounded by |x| / 2 times the erf error"
    gf = np.abs(X.gelu_fast64(x) - X.gelu64(x))
    inside = np.abs(x) <= 8.0
    _three_figures(gf[inside].max(), 2.52e-5, "gelu_fast abs error on [-8, 8]")
    # outside the fitted range the maximum sits just past |x| = 8, where the two sweeps have different points: one figure each
    _three_figures(gf[~inside].max(), {"bf16_all": 6.59e-12, "f32_grid": 8.11e-12}[sweep], "gelu_fast abs error outside [-8, 8]")
    fd = np.abs(X.gelu_fast_grad64(x) - X.gelu_grad64(x))
    _three_figures(fd.max(), 1.10e-4, "gelu_fast' against the erf form")
    assert abs(abs(x[fd.argmax()]) - 0.93) < 0.01 and fd.max() <= X.MIXED_PAIR_CLAIM
    eg = np.abs(X.gelu_erf_grad64(x) - X.gelu_grad64(x))
    _three_figures(eg.max(), 6.97e-8, "gelu_erf_grad against the erf form")
    mixed = np.abs(X.gelu_erf_grad64(x) - X.gelu_fast_grad64(x))
    _three_figures(mixed.max(), 1.10e-4, "gelu_erf_grad against d(gelu_fast)")
    assert mixed.max() <= X.MIXED_PAIR_CLAIM


def test_negative_tail_of_gelu_erf_is_absolutely_not_relatively_accurate():
    """pytc_common.h: the A&S tail goes as 0.778 / z against 1 / (sqrt(pi) z) -- the relative error for x < 0 reaches 0.44 over the
    bf16 values while the absolute error stays under 2.12e-7"""
    x = _finite_bf16().astype(D)
    x = x[x < 0]
    ref, got = X.gelu64(x), X.gelu_erf64(x)
    ok = ref != 0
    rel = np.abs(got[ok] - ref[ok]) / np.abs(ref[ok])
    print(f"relative error of gelu_erf for x < 0: {rel.max():.4f} at x = {x[ok][rel.argmax()]}")
    assert 0.44 <= rel.max() <= 0.45
    assert np.abs(got - ref).max() <= 2.12e-7
    z = -30.0 * np.sqrt(0.5)                                                 # the tail constants
    t = 1.0 / (1.0 + X.AS_C[0] * -z)
    assert abs(X.AS_C[5] / X.AS_C[0] - 0.778) < 5e-4 and abs(X._as_one_plus_erf64(np.array([z]))[0] / (np.exp(-z * z) * t) - X.AS_C[5]) < 0.02


# ------------------------------------------------------------------------------------------------------------ models against fp64
@pytest.mark.parametrize("fn", ["gelu_erf", "gelu_erf_grad", "gelu_fast", "gelu_fast_grad", "gelu_grad_libm"])
def test_fp32_models_restate_the_fp64_formulas(fn):
    """the un-nudged fp32 model is the fp64 formula up to fp32 rounding of its steps (a transcription error would show as 1e-4 .. 1)"""
    x = X.f32_grid().ravel()
    got = X.MODELS[fn][0](x).astype(D)
    want = X.FUNCTION64[fn](x.astype(D))
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"{fn}: fp32 model against its fp64 formula, max scaled error {err.max():.3e}")
    # erf forms: a handful of fp32 roundings of O(1) terms.  gelu_fast forms: the exponent u = x p(x^2) is rounded to fp32 before 2^u, a
    # relative error 2^-24 |u| ln 2 of e, and g' multiplies it by |x du/dx| (up to ~10 where s (1 - s) is not negligible): ~2e-6
    assert err.max() <= (4e-6 if fn.startswith("gelu_fast") else 4e-7)


def test_sigmoid_and_tanh_models():
    x = X.f32_grid().ravel()
    with np.errstate(all="ignore"):
        assert np.abs(X.sigmoid(x).astype(D) - 1.0 / (1.0 + np.exp(-x.astype(D)))).max() <= 2e-7
        assert np.abs(X.tanh(x).astype(D) - np.tanh(x.astype(D))).max() <= 6e-8


@pytest.mark.parametrize("fn", list(X.MODELS))
def test_intervals_contain_the_central_model_and_are_narrow(fn):
    x = X.bf16_all()
    for out in ("f32", "bf16"):
        iv = X.interval(fn, x, out=out)
        assert X.inside(iv, X.store(X.MODELS[fn][0](x), out)).all()
        fin = np.isfinite(iv.lo) & np.isfinite(iv.hi)
        with np.errstate(all="ignore"):
            width = (iv.hi.astype(D) - iv.lo.astype(D))[fin]
            xs = np.maximum(1.0, np.abs(x[fin].astype(D)))
            top = np.maximum(np.abs(iv.hi), np.abs(iv.lo))[fin]
        # Every function here is a sum of at most three terms of size <= max(1, |x|), each carrying the (2 B + 1) <= 7 units of one or two
        # transcendentals (unit 2^-24 relative) plus the one-ulp widening: an fp32 interval is narrower than 2e-6 max(1, |x|), fifty times
        # below the smallest seeded defect (1e-4).  Measured: 4.2e-7 (gelu_erf) ... 1.3e-6 (gelu_fast_grad).  Stored as bf16 the two ends
        # may in addition round to neighbouring bf16 values: one bf16 ulp of the larger end.
        limit = 2.0e-6 * xs
        if out == "bf16":
            limit = limit + np.spacing(top.astype(np.float32)).astype(D) * 65536.0
        worst = (width / limit).max()
        print(f"{fn} -> {out}: widest interval {worst:.3f} of its limit")
        assert worst <= 1.0, f"{fn} -> {out}: interval width {worst:.3f} of the limit"


# ------------------------------------------------------------------------------------------------------------ pairing table
@pytest.mark.parametrize("p", X.PAIRINGS, ids=[p.schedule for p in X.PAIRINGS])
def test_backward_differentiates_what_the_forward_evaluated(p):
    for name, sweep in SWEEPS.items():
        x = sweep().astype(D)
        analytic = X.DERIVATIVE64[p.forward](x)
        # central differences of the forward's own formula (not across the clamp of gelu_fast at |x| = 8, not where h is below an ulp)
        h = 1e-6 * np.maximum(1.0, np.abs(x))
        ok = (np.abs(x) < 1e6) & (np.abs(np.abs(x) - 8.0) > 2e-5)
        cd = (X.FUNCTION64[p.forward](x + h) - X.FUNCTION64[p.forward](x - h)) / (2.0 * h)
        assert np.abs(cd - analytic)[ok].max() <= 1e-9, f"{p.forward}: the analytic derivative is not the derivative"
        gap = np.abs(X.FUNCTION64[p.backward](x) - analytic).max()
        print(f"{p.schedule} [{name}]: forward {p.forward}, backward {p.backward}: max |f'_applied - d f_forward| = {gap:.4e}")
        assert gap <= p.bound
        if p.same:
            assert gap <= 6e-7, "a same-function pair differs by more than the A&S slope error"
        else:
            assert p.bound == X.MIXED_PAIR_CLAIM and gap >= 1e-4, "a mixed pair must be named as one"
    if p.same and p.bound > 1e-9:
        _three_figures(np.abs(X.FUNCTION64[p.backward](SWEEPS["f32_grid"]().astype(D)) - X.DERIVATIVE64[p.forward](SWEEPS["f32_grid"]().astype(D))).max(),
                       p.bound, p.schedule)


def test_pairing_rows_name_functions_the_entry_table_files():
    fwd = {e.fn for e in X.ENTRIES}
    for p in X.PAIRINGS:
        assert p.forward in fwd and p.backward in X.MODELS
    # the pw_wgrad_dgrad rows of the two tables agree: C_in = 32 / 64 multiply by gelu_erf_grad, the wide kernel by gelu_fast's own derivative
    assert X.BY_ID["pw_wgrad_dgrad.32.dhp"].fn == X.BY_ID["pw_wgrad_dgrad.64.dhp"].fn == "gelu_erf_grad"
    assert X.BY_ID["pw_wgrad_dgrad.128.dhp"].fn == "gelu_fast_grad"


# ------------------------------------------------------------------------------------------------------------ discrimination
def _escapes(fn, xs, *, mid, out, defect=None, alt_fn=None, alt_mid="same") -> int:
    """inputs at which the changed model's value lies outside the real model's interval"""
    iv = X.interval(fn, xs, mid=mid, out=out)
    v = X.MODELS[alt_fn or fn][0](xs, defect=defect)
    if (mid if alt_mid == "same" else alt_mid) == "bf16":
        v = X.round_bf16(v)
    return int((~X.inside(iv, X.store(v, out))).sum())


# (what, real function, kwargs of _escapes, sweep): every sweep named here is one a table row of that function and rounding runs
SEEDED = [
    ("A&S coefficient 0.3275911 -> 0.3275912", "gelu_erf", dict(mid=None, out="f32", defect="as_coef"), "f32_grid"),
    ("gelu_fast coefficient 1.0142630e-3 -> 1.0142631e-3", "gelu_fast", dict(mid="bf16", out="bf16", defect="fast_coef"), "bf16_all"),
    ("gelu_fast' coefficient 1.0142630e-3 -> 1.0142631e-3", "gelu_fast_grad", dict(mid=None, out="bf16", defect="fast_coef"), "bf16_all"),
    ("clamp of x^2 at 64 removed (g)", "gelu_fast", dict(mid="bf16", out="bf16", defect="no_clamp"), "bf16_all"),
    ("clamp of x^2 at 64 removed (g')", "gelu_fast_grad", dict(mid=None, out="bf16", defect="no_clamp"), "bf16_all"),
    ("1 - s replaced by e * s", "gelu_fast_grad", dict(mid=None, out="bf16", defect="e_times_s"), "bf16_all"),
    ("bf16 rounding of the activation dropped", "gelu_fast", dict(mid="bf16", out="f32", alt_mid=None), "bf16_all"),
    ("bf16 rounding of the activation added", "gelu_erf", dict(mid=None, out="f32", alt_mid="bf16"), "bf16_all"),
    ("gelu_erf swapped for gelu_fast (bf16 operand)", "gelu_erf", dict(mid="bf16", out="bf16", alt_fn="gelu_fast"), "bf16_all"),
    ("gelu_erf swapped for gelu_fast (fp32)", "gelu_erf", dict(mid=None, out="f32", alt_fn="gelu_fast"), "bf16_all"),
    ("gelu_fast swapped for gelu_erf", "gelu_fast", dict(mid="bf16", out="bf16", alt_fn="gelu_erf"), "bf16_all"),
    ("gelu_erf_grad swapped for gelu_fast'", "gelu_erf_grad", dict(mid=None, out="bf16", alt_fn="gelu_fast_grad"), "bf16_all"),
    ("gelu_fast' swapped for gelu_erf_grad", "gelu_fast_grad", dict(mid=None, out="bf16", alt_fn="gelu_erf_grad"), "bf16_all"),
    ("erff swapped for the A&S form (fp32)", "gelu_grad_libm", dict(mid=None, out="f32", defect="as_erf"), "bf16_all"),
    ("erff swapped for the A&S form (bf16)", "gelu_grad_libm", dict(mid=None, out="bf16", defect="as_erf"), "bf16_all"),
]


@pytest.mark.parametrize("what,fn,kw,sweep", SEEDED, ids=[s[0] for s in SEEDED])
def test_seeded_change_leaves_the_interval(what, fn, kw, sweep):
    assert any(e.fn == fn and sweep in e.sweep and e.dout == kw["out"] and (e.mid == kw["mid"]) for e in X.ENTRIES), \
        f"no table row runs {fn} (mid {kw['mid']}, out {kw['out']}) over {sweep}"
    n = _escapes(fn, SWEEPS[sweep](), **kw)
    print(f"{what}: outside the interval of {fn} at {n} inputs of {sweep}")
    assert n >= 1


def test_x_le_0_is_not_a_change():
    """`x < 0` taken as `x <= 0` differs only at x = +-0, where p(t) exp2(0) = p(1) is EXACTLY 1.0f (the five A&S coefficients sum to
    1 in fp32): pe = 2 - pe, and both forms give the same bits for every input.  No test can see it because there is nothing to see."""
    p, e = X._as_parts(np.zeros(1, np.float32), 0, 0, None)
    assert (p * e)[0] == np.float32(1.0) and (np.float32(2.0) - p * e)[0] == np.float32(1.0)
    for x in (X.bf16_all(), X.f32_grid()):
        for f in (X.gelu_erf, X.gelu_erf_grad):
            assert np.array_equal(f(x, defect="le").view(np.uint32), f(x).view(np.uint32))


def test_as_coefficients_other_than_the_first_round_to_the_same_float():
    """a change in the last printed digit of the five polynomial coefficients is below fp32 resolution: the constant in the object code is
    the same, so the seeded coefficient change uses 0.3275911"""
    for c, step in zip(X.AS_C[1:], (1e-9,) * 5):
        assert np.float32(c) == np.float32(c + step) or np.float32(c) == np.float32(c - step)
    assert np.float32(X.AS_C[0]) != np.float32(X.AS_C[0] + 1e-7)


# ------------------------------------------------------------------------------------------------------------ class rules
def test_class_rules_of_the_models():
    x = X.bf16_all()
    fin, nan = np.isfinite(x), np.isnan(x)
    pz, nz = x.ravel().view(np.uint32) == 0, x.ravel().view(np.uint32) == 0x80000000
    for fn in X.MODELS:
        for out in ("f32", "bf16"):
            iv = X.interval(fn, x, out=out)
            assert not iv.nan_ok[fin].any() and np.isfinite(iv.lo[fin]).all() and np.isfinite(iv.hi[fin]).all(), f"{fn}: a finite input may give NaN / inf"
            assert iv.nan_ok[nan].all() and not iv.num_ok[nan].any(), f"{fn}: NaN in must give NaN out"
    for fn in ("gelu_erf", "gelu_fast"):                        # +-0 in, +-0 out
        v = X.MODELS[fn][0](x).ravel()
        assert (v[pz].view(np.uint32) == 0).all() and (v[nz].view(np.uint32) == 0x80000000).all()
    for fn in ("gelu_erf_grad", "gelu_fast_grad", "gelu_grad_libm"):
        zeros = np.array([0.0, -0.0], dtype=np.float32)
        for k0 in (-2, 0, 2):                                   # rcp(1), exp2(0), erff(0) are exact cases: no nudge moves them
            for k1 in (-2, 0, 2):
                assert (X.MODELS[fn][0](zeros, k0, k1) == np.float32(0.5)).all(), f"{fn}(+-0) must be exactly 1/2"
    # the +-inf classes are those of the fp64 formulas 0.5 x (1 + erf) and Phi + x phi: f(+inf) = +inf, f(-inf) = -inf * 0 = NaN, f'(+-inf) = NaN
    # (inf * 0); torch.nn.functional.gelu returns the same.  No table row documents another value.
    inf = np.array([np.inf, -np.inf], dtype=np.float32)
    with np.errstate(all="ignore"):
        for fn, ref in (("gelu_erf", X.gelu64), ("gelu_fast", X.gelu64), ("gelu_erf_grad", X.gelu_grad64), ("gelu_fast_grad", X.gelu_grad64),
                        ("gelu_grad_libm", X.gelu_grad64)):
            got, want = X.MODELS[fn][0](inf), ref(inf.astype(D))
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)]), f"{fn}(+-inf) = {got}"
        assert np.array_equal(X.sigmoid(inf), [1.0, 0.0]) and np.array_equal(X.tanh(inf), [1.0, -1.0])


# ------------------------------------------------------------------------------------------------------------ isolation premises
def _premise(e, sweep):
    """the fp64 reference of the GEMM around the activation, with the activation replaced by the identity / by 1: it must hand the swept
    values (or the constant 1) through unchanged, every output a sum with at most one non-zero term"""
    with np.errstate(invalid="ignore"):
        x = X.sweep_values(e, sweep).astype(D)
    xf = np.where(np.isfinite(x), x, 0.0)
    r = e.recipe
    if r in ("elementwise",):
        return
    if r == "grn":                                               # fmaf(dh2, A, h * B) with dh2 = A = 1, B = 0
        assert np.array_equal(1.0 * 1.0 + xf * 0.0, np.ones_like(xf))
    elif r == "ones_times_grad":
        cin = {32: 32, 128: 64}[e.width]
        w = X.zero_padded_identity(e.width, cin)
        y = X.one_term_gemm(np.ones((x.shape[0], cin)), w)
        assert y.shape == x.shape and np.array_equal(y, np.ones_like(x))
    elif r in ("identity_after", "identity_before"):
        cout = 128 if e.width == 64 else e.width
        w = X.top_identity(cout, e.width)
        y = X.one_term_gemm(xf, w)
        assert np.array_equal(y[:, :e.width], xf) and not y[:, e.width:].any()
    elif r == "stem":
        y = X.one_term_gemm(xf, np.ones((8, 1)))
        assert all(np.array_equal(y[:, j], xf[:, 0]) for j in range(8))
    elif r == "head":
        a = np.zeros((x.shape[0], 8))
        a[:, 0] = xf[:, 0]
        w = np.zeros((1, 8))
        w[0, 0] = 1.0
        assert np.array_equal(X.one_term_gemm(a, w)[:, 0], xf[:, 0])
    elif r == "mixer":
        hp = X.one_term_gemm(xf, X.top_identity(64, 32))                  # expand: x beside 32 zero channels (gelu_fast(0) = 0 exactly)
        assert np.array_equal(hp[:, :32], xf) and not hp[:, 32:].any() and X.gelu_fast(np.zeros(1, np.float32))[0] == 0
        y = X.one_term_gemm(hp, X.top_identity(64, 32).T)                 # project: the first 32 hidden channels
        assert np.array_equal(y, xf)
    elif r == "rebuilt":
        chid = int(e.id.split(".")[1])
        hp = X.one_term_gemm(xf[:32], X.zero_padded_identity(chid, 32))       # the rebuilt pre-activation: t in every 32-channel group
        assert all(np.array_equal(hp[:, g:g + 32], xf[:32]) for g in range(0, chid, 32))
        assert np.array_equal(X.one_term_gemm(np.eye(32).T, hp.T), hp)         # dW3 = dy^T g(hp)
        assert np.array_equal(X.one_term_gemm(np.eye(32), np.ones((32, chid)).T), np.ones((32, chid))) and x.shape[0] % 32 == 0
    elif r == "onehot_wgrad":
        rows = 32 if e.id.startswith("pw_wgrad_dgrad") else 64
        assert e.id.startswith(("pw_wgrad", "linear_bwd.plain.dW"))
        for blk in (xf[:rows], xf[-rows:]):
            y = X.one_term_gemm(np.eye(rows).T, blk.T)           # dW = dy^T g(x): (rows, rows) @ (rows, K)
            assert np.array_equal(y, blk)
        assert x.shape[0] % rows == 0
    elif r == "onehot_row":
        dy = np.zeros((4, 32))
        dy[:, 0] = 1.0
        w3 = np.zeros((32, 64))
        w3[0, :] = 1.0
        assert np.array_equal(X.one_term_gemm(dy, w3.T), np.ones((4, 64))) and e.width == 64      # (W3^T dy)[r][k] = sum_o dy[r][o] W3[o][k]
    elif r == "onehot_dgrad":
        y = X.one_term_gemm(np.eye(32), np.ones((32, e.width)).T)        # (W^T dy)[r][k] = sum_o dy[r][o] W[o][k]
        assert np.array_equal(y, np.ones((32, e.width))) and x.shape[0] % 32 == 0
    else:
        raise AssertionError(f"no premise for recipe {r}")


@pytest.mark.parametrize("e", X.ENTRIES, ids=[e.id for e in X.ENTRIES])
def test_operands_isolate_the_activation(e):
    assert e.fn in X.MODELS and e.recipe in X.RECIPES and e.din in ("f32", "bf16") and e.dout in ("f32", "bf16")
    assert ("f32_grid" in e.sweep) == (e.din == "f32"), "fp32 routes sweep the fp32 grid as well, bf16 routes cannot hold it"
    for sweep in e.sweep:
        x = X.sweep_values(e, sweep)
        assert x.size in (1 << 16, 1 << 19) and x.shape[1] == e.width
        if e.din == "bf16":
            assert not (x.view(np.uint32) & 0xFFFF).any()
        assert e.spec.shares_sum == bool(np.isfinite(x).all() and sweep == "bf16_all") or sweep == "f32_grid"
        _premise(e, sweep)


# the groups the issue lists, each bit-identical without tolerance (plus the rows found to belong to them): every set must lie inside ONE group
PROMISED_GROUPS = {
    "gelu_erf, fp32": {"gelu.fwd.f32", "pw_conv.act.gelu.generic.f32", "pw_conv.pre_act.generic.f32", "linear_fwd.plain.f32", "pw_wgrad.valu.f32",
                       "linear_bwd.plain.dW"},
    "gelu_erf, bf16": {"gelu.fwd.bf16", "pw_conv.act.gelu.generic.bf16", "pw_conv.act.gelu.stem", "pw_conv.act.gelu.head", "pw_conv.pre_act.generic.bf16",
                       "linear_fwd.plain.bf16", "pw_wgrad.valu.bf16"},
    "gelu_fast rounded to bf16": {"pw_conv.pre_act.paired", "pw_conv.pre_act.rowmajor", "linear_fwd.mfma", "pw_mlp.train.stored", "pw_mlp.train.nostore",
                                  "pw_wgrad.mfma", "mixer_bwd_rc.32.dW3", "mixer_bwd_rc.64.dW3", "pw_wgrad_dgrad.32.dW", "pw_wgrad_dgrad.64.dW",
                                  "pw_wgrad_dgrad.128.dW"},
    "gelu_erf_grad, bf16": {"pw_conv.res_gelu_bwd.generic.bf16", "pw_conv.res_gelu_bwd.paired", "pw_conv.res_gelu_bwd.rowmajor", "linear_bwd.plain.bf16",
                            "linear_bwd.mfma", "pw_mlp_bwd.d_hidden", "pw_wgrad_dgrad.32.dhp", "pw_wgrad_dgrad.64.dhp"},
    "gelu_erf_grad, fp32": {"pw_conv.res_gelu_bwd.generic.f32", "linear_bwd.plain.f32"},
    "gelu_fast_with_grad": {"mixer_bwd_rc.32.dhp", "mixer_bwd_rc.64.dhp", "pw_wgrad_dgrad.128.dhp"},
}


def test_same_function_groups_are_the_ones_the_table_promises():
    groups = {}
    for e in X.ENTRIES:
        groups.setdefault(e.group, set()).add(e.id)
    for name, want in PROMISED_GROUPS.items():
        assert want <= set(X.BY_ID), f"{name}: unknown rows {want - set(X.BY_ID)}"
        keys = {X.BY_ID[i].group for i in want}
        assert len(keys) == 1, f"{name}: its rows fall into {len(keys)} groups {keys} and would never be compared with each other"
        assert groups[keys.pop()] == want, f"{name}: the group also holds {groups[X.BY_ID[next(iter(want))].group] - want}"
    # rows alone in their group are alone for a reason: the only row of their function, type and rounding
    alone = {next(iter(v)) for v in groups.values() if len(v) == 1}
    assert alone == {"pw_conv.act.sigmoid.generic.f32", "pw_conv.act.tanh.generic.f32", "linear_bwd.plain.dW.bf16"}
    assert "ops.pw_mlp_bwd" not in X.NOT_COVERED and "ops.pw_mlp_up" in X.NOT_COVERED


def test_design_document_lists_every_row():
    text = (Path(__file__).resolve().parent.parent / "DESIGN.md").read_text()
    for e in X.ENTRIES:
        assert f"`{e.id}`" in text, f"DESIGN.md 4.3c does not list {e.id}"
    for p in X.PAIRINGS:
        assert p.schedule in text, f"DESIGN.md 4.3c does not list the schedule {p.schedule}"
    for k in X.NOT_COVERED:
        assert k in text


def test_budgets_are_the_probe_files():
    """the constants cite profiles/activation_domain_probe.txt: its "budget" lines must say the same"""
    import re
    text = (Path(__file__).resolve().parent.parent / "profiles" / "activation_domain_probe.txt").read_text()
    found = {m.group(1): int(m.group(2)) for m in re.finditer(r"^budget (\w+)\s*= (\d+)", text, re.M)}
    for k in ("exp2", "rcp", "erff", "tanhf"):
        assert found[k] == X.BUDGET[k], f"budget of {k}: probe file {found[k]}, case module {X.BUDGET[k]}"
    assert X.EXPF_IS_EXP2_OF_PRODUCT and X.BUDGET["expf"] == X.BUDGET["exp2"]
    assert len(re.findall(r"__expf\(v\) != v_exp_f32\(v \* log2e\) at 0 arguments", text)) == 3
    assert len(re.findall(r"exact cases.*reference: 0$", text, re.M)) == 5

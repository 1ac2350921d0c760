"""Footprint cases of the training-step (backward) launches: for every C ABI entry of csrc/train_kernels.hip that writes memory, and for
the four dense weight-gradient entries with workspaces, the operands, the fp64 reference of every output and the element ranges of
every buffer that include/pytc_hip.h documents as written -- for slot workspaces as a function of *slots_out.

Plain module, host only (no GPU import): tests/test_gpu_train_footprint.py runs the cases inside sentinel-filled guard bands through the
raw ABI, tests/test_host_train_footprint_cases.py checks the table itself (edges reached, caps, an independent autograd reference per
family, completeness against the sources).

Operands come from the exact builders of exact_reduction_cases.py: ternary / binary values, exact affines, GELU pre-activations in
{0, 16}, mean in {-1, 0, 1}, rstd and count powers of two, gamma a signed power of two.  Every product and every partial sum is then an
fp32 number in any order (the caps are asserted when a case is built: assert_exact_cap / gemm_abs_bound), so every comparison is bit
equality with fp64; no tolerance is measured anywhere.  (The mixer cases need a = gamma * rstd = +-16 to keep the hidden pre-activation
in {0, 16}, so their gamma is +-16 / rstd, still a signed power of two.)

One output is not exact in its storage type and is compared with the fp64 reference ROUNDED ONCE to that type:
  * `dt` of pytc_norm_bwd in bf16: dt = rstd gamma (dtn - S1 / count - xhat S2 / count) with S1, S2 the launch's own sums over the
    drawn operands -- integers (half-integers) with up to ~12 significant bits, more than bf16 holds.  The fp32 value before the store
    is exact, so the single rounding is the store's; the comparison allows the one unit in the last place the rule grants and the
    GPU case reports how many elements used it.
pytc_norm_bwd_apply takes its sums as an operand: they are chosen (count x {0, +-1/2, +-1}) so that dt is a bf16 number.  The entry
refuses rows that are no multiple of 16 bytes (C % 8 for bf16, C % 4 for fp32), so its narrow bf16 case is C = 8 where the other norm
launches run bf16 C = 12; fp32 C = 12, bf16 C = 32 and fp32 C = 32 are as everywhere.

Knobs.  Every case lists the knob forms its launch reads (KNOB_DEFAULTS names them with the library's defaults, which a host test
compares with the table of csrc/pytc_common.h).  `elementwise_vec` is in that list for completeness only: the launches that read it
(pytc_affine_act, pytc_act_bwd, pytc_norm_bwd_apply_general) belong to the dense-conv units, not to these families, so no case here has a
form for it.  pytc_act_norm_bwd_apply / pytc_act_norm_bwd_apply_cg (csrc/rsunet_train_kernels.hip) are outside this table as well:
the `_cg` form is still launched by no test and has no guarded case after this module either.

Edges.  Every family with row slots has a slot count above one, a ragged last slot and a row count that is no multiple of 32; the
forms whose slots may straddle samples (pw_wgrad*, pw_wgrad_dgrad) have N > 1 with a slot and a 32-row block across a sample boundary
(mixer_bwd_rc, pw_wgrad_groupnorm, the norm and depthwise launches split rows per sample by construction).  The empty-last-slot case
(66 049 = 257^2 rows, N = 1: 258 slots of 257 rows, the last one without a row) exists for pw_wgrad bf16 32 -> 64 (matrix-core form),
fp32 8 -> 8 (generic form), pw_wgrad_dgrad 64 -> 32, mixer_bwd_rc and pw_wgrad_groupnorm; the norm launches have empty slots there as
well (1024 slots of 65 rows: 1017 used).  The 1024-slot cap is reached at 262 144 + 37 rows by the generic pw_wgrad form (fp32 8 -> 8;
257 rows per slot leave three empty slots) and by the norm statistics.  The matrix-core weight-gradient forms launch at most
min(1024, rows / 2048) slots and the depthwise forms need more than two million positions for 1024 slots: their cap is out of reach
of a quick test and no case claims it.  The dense weight gradients have no mirror: the GPU case asserts that the library's own
workspace holds more than one slot."""
from __future__ import annotations

import functools
import sys
from dataclasses import dataclass, field
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import exact_reduction_cases as X  # noqa: E402

GUARD = 4096                      # elements either side of every payload (tests/test_gpu_mixer_exact.py)
SENTINEL_F32 = 0x7FC5A5A5         # a quiet NaN with a recognisable payload, compared by bits
SENTINEL_16 = 0x7FC5              # ... in bf16
BF16, F32 = torch.bfloat16, torch.float32

# knob -> library default (csrc/pytc_common.h); the GPU cases restore these after every form
KNOB_DEFAULTS = {"wgrad_valu": 0, "wgrad_small_split": 1, "wgrad_whole_rounds": 1, "wgrad_dgrad_fused": 1, "mixer_bwd_rc_slot_div": 1,
                 "dw_wgrad_march": 1, "dw_wgrad_vec": 1, "conv_wgrad_mfma": 1, "norm_bwd_from_wgrad_flat": 1, "elementwise_vec": 1}

# entries of csrc/train_kernels.hip (and the dense weight-gradient files) that need no footprint case, with the reason
EXEMPT = {
    "pytc_pw_wgrad_slots": "host query (workspace bound), writes no device memory",
    "pytc_pw_wgrad_dgrad_supported": "host query",
    "pytc_pw_wgrad_groupnorm_sps": "host query",
    "pytc_pw_wgrad_groupnorm_supported": "host query",
    "pytc_pw_wgrad_groupnorm_ws_elems": "host query; every groupnorm case sizes its workspace by it",
    "pytc_mixer_bwd_rc_supported": "host query",
    "pytc_mixer_bwd_rc_sps": "host query",
    "pytc_mixer_bwd_rc_ws_elems": "host query; every mixer case sizes its workspace by it",
    "pytc_dw_wgrad_slots": "host query",
    "pytc_norm_bwd_ws_elems": "host query",
    "pytc_conv3d_wgrad_ws_elems": "host query",
    "pytc_conv3d_wgrad_strided_ws_elems": "host query",
    "pytc_upcat_deconv2_wgrad_ws_elems": "host query",
    "pytc_dwconv3d_bwd_data": "footprint guarded in tests/test_gpu_stencil_exact.py (NaN-filled buffers with guard rows)",
    "pytc_dwconv3d_bwd_data_add": "footprint guarded in tests/test_gpu_stencil_exact.py",
    "pytc_layernorm_rows_bwd": "footprint guarded in tests/test_gpu_layernorm_exact.py",
    "pytc_layernorm_wide_bwd": "footprint guarded in tests/test_gpu_layernorm_exact.py",
    "pytc_layernorm_any_bwd": "footprint guarded in tests/test_gpu_layernorm_exact.py",
    "pytc_act_norm_bwd_stats": "footprint guarded in tests/test_gpu_norm_act_exact.py",
    "pytc_reduce_slots_multi": "run by every *_partial case and by the item-count cases of test_gpu_train_footprint.py (REDUCE_ENTRY)",
}
REDUCE_ENTRY = "pytc_reduce_slots_multi"
DENSE_ENTRIES = ("pytc_conv3d_wgrad", "pytc_conv3d_wgrad_strided", "pytc_upcat_deconv2_wgrad", "pytc_deconv2_upfirst_wgrad")


# ------------------------------------------------------------------------------------------------------------------ the table
@dataclass(frozen=True)
class Case:
    id: str
    family: str                 # pw | mixer | norm | dw | elementwise | dense
    entry: str                  # the C ABI entry the case launches
    p: tuple                    # ((name, value), ...) parameters; dict(case.p)
    forms: tuple = ()           # knob forms: (((knob, value), ...), ...): each must give the default form's bits and footprint
    edges: tuple = ()           # the edges the case claims (test_host_train_footprint_cases.py verifies them by the mirrors)

    def __getitem__(self, k):
        return dict(self.p)[k]

    def get(self, k, default=None):
        return dict(self.p).get(k, default)


@dataclass
class Ref:
    """reference of one output: fp64 values in the output's shape; `ulp` > 0 only for the outputs the module docstring names"""
    dtype: torch.dtype
    ref: torch.Tensor
    ulp: int = 0


@dataclass
class Region:
    """a documented slot-partial region of a workspace: [offset, offset + slots * n) floats laid out [slots][n]; `total` (fp64, n
    values) is what the region must sum to over its slots; written = False: the header documents it as NOT written in this form"""
    name: str
    offset: int
    slots: int
    n: int
    total: torch.Tensor | None
    written: bool = True


@dataclass
class Built:
    inputs: dict                                  # name -> CPU tensor (operands, in their storage type)
    outputs: dict                                 # name -> Ref
    totals: dict = field(default_factory=dict)    # name -> fp64 totals of the slot-partial regions
    inout: dict = field(default_factory=dict)     # name -> CPU tensor an in-place output starts from


def _c(id, family, entry, forms=(), edges=(), **p):
    return Case(id, family, entry, tuple(sorted(p.items())), tuple(tuple(sorted(f.items())) for f in forms), tuple(edges))


def _dtn(dt):
    return "bf16" if dt == BF16 else "fp32"


PW_KNOBS = ({"wgrad_valu": 1}, {"wgrad_small_split": 0}, {"wgrad_whole_rounds": 0})
EMPTY_ROWS = 257 * 257                      # 66 049: 258 slots of 257 rows, the last one empty
CAP_ROWS = 262144 + 37                      # 1024 slots of 257 rows: 1021 used


def _pw_cases():
    out = []
    small = dict(N=3, rows=347)                                   # 1041 rows: 4 slots of 261, last 258; 347 % 32 = 27; slots straddle
    e_small = ("slots>1", "ragged", "rows%32", "straddle")
    for entry in ("pytc_pw_wgrad", "pytc_pw_wgrad_partial"):
        t = "imm" if entry == "pytc_pw_wgrad" else "part"
        out += [
            _c(f"pw_{t}_bf16_32x64_ab_db", "pw", entry, PW_KNOBS, e_small + ("mfma",), dtype=BF16, c_in=32, c_out=64, ab=1, gelu=0, want_db=1, **small),
            _c(f"pw_{t}_bf16_64x32_gelu_nodb", "pw", entry, PW_KNOBS, e_small + ("mfma",), dtype=BF16, c_in=64, c_out=32, ab=0, gelu=1, want_db=0, **small),
            _c(f"pw_{t}_bf16_24x40_ab_db", "pw", entry, (), e_small + ("valu",), dtype=BF16, c_in=24, c_out=40, ab=1, gelu=0, want_db=1, **small),
            _c(f"pw_{t}_bf16_40x24_gelu_db", "pw", entry, (), e_small + ("valu",), dtype=BF16, c_in=40, c_out=24, ab=0, gelu=1, want_db=1, **small),
            _c(f"pw_{t}_fp32_8x8_ab_nodb", "pw", entry, (), e_small + ("valu",), dtype=F32, c_in=8, c_out=8, ab=1, gelu=0, want_db=0, **small),
            _c(f"pw_{t}_fp32_12x20_gelu_db", "pw", entry, (), e_small + ("valu",), dtype=F32, c_in=12, c_out=20, ab=0, gelu=1, want_db=1, **small),
            _c(f"pw_{t}_bf16_thin_1x16_db", "pw", entry, (), e_small + ("thin",), dtype=BF16, c_in=1, c_out=16, ab=0, gelu=0, want_db=1, **small),
            _c(f"pw_{t}_bf16_thin_16x1_db", "pw", entry, (), e_small + ("thin",), dtype=BF16, c_in=16, c_out=1, ab=0, gelu=0, want_db=1, **small),
            _c(f"pw_{t}_fp32_thin_8x1_nodb", "pw", entry, (), e_small + ("thin",), dtype=F32, c_in=8, c_out=1, ab=0, gelu=0, want_db=0, **small),
            _c(f"pw_{t}_bf16_32x64_empty_last_slot", "pw", entry, ({"wgrad_valu": 1},), ("slots>1", "empty_last", "rows%32", "mfma"),
               dtype=BF16, c_in=32, c_out=64, ab=0, gelu=0, want_db=1, N=1, rows=EMPTY_ROWS),
            _c(f"pw_{t}_fp32_8x8_empty_last_slot", "pw", entry, (), ("slots>1", "empty_last", "rows%32", "valu"),
               dtype=F32, c_in=8, c_out=8, ab=0, gelu=0, want_db=1, N=1, rows=EMPTY_ROWS),
            _c(f"pw_{t}_fp32_8x8_cap1024", "pw", entry, (), ("slots>1", "cap1024", "rows%32", "valu"),
               dtype=F32, c_in=8, c_out=8, ab=0, gelu=0, want_db=1, N=1, rows=CAP_ROWS),
        ]
    for ci in (32, 64, 128):
        out.append(_c(f"pw_dgrad_{ci}x32_db", "pw", "pytc_pw_wgrad_dgrad_partial", PW_KNOBS[1:], e_small + ("mfma",),
                      dtype=BF16, c_in=ci, c_out=32, ab=0, gelu=1, want_db=1, **small))
    out.append(_c("pw_dgrad_64x32_nodb", "pw", "pytc_pw_wgrad_dgrad_partial", (), e_small + ("mfma",),
                  dtype=BF16, c_in=64, c_out=32, ab=0, gelu=1, want_db=0, **small))
    out.append(_c("pw_dgrad_64x32_empty_last_slot", "pw", "pytc_pw_wgrad_dgrad_partial", (), ("slots>1", "empty_last", "rows%32", "mfma"),
                  dtype=BF16, c_in=64, c_out=32, ab=0, gelu=1, want_db=1, N=1, rows=EMPTY_ROWS))
    return out


def _mixer_cases():
    out = []
    two = dict(N=2, rows=701)           # 1402 rows: 5 slots -> 2 per sample of 351 rows, last 350; 701 % 32 = 29
    e_two = ("slots>1", "ragged", "rows%32", "sps>1")
    flat = ({"norm_bwd_from_wgrad_flat": 0},)
    for hid in (32, 64, 96):
        for gn in ((0, 1) if hid != 96 else (0,)):
            for db3 in (0, 1):
                out.append(_c(f"mixer_hid{hid}_gn{gn}_db{db3}", "mixer", "pytc_mixer_bwd_rc", flat if gn else (), e_two,
                              c_hid=hid, gn=gn, want_db3=db3, **two))
    out.append(_c("mixer_hid64_gn1_sps1", "mixer", "pytc_mixer_bwd_rc", (), ("slots>1", "rows%32", "sps==1"),
                  c_hid=64, gn=1, want_db3=1, N=3, rows=347))
    out.append(_c("mixer_hid64_gn1_empty_last_slot", "mixer", "pytc_mixer_bwd_rc", ({"mixer_bwd_rc_slot_div": 2},),
                  ("slots>1", "empty_last", "rows%32", "sps>1"), c_hid=64, gn=1, want_db3=1, N=1, rows=EMPTY_ROWS))
    out.append(_c("gn_32x64_sps1", "mixer", "pytc_pw_wgrad_groupnorm", flat, ("slots>1", "rows%32", "sps==1"), c=32, c_hid=64, N=3, rows=347))
    out.append(_c("gn_32x64_sps2", "mixer", "pytc_pw_wgrad_groupnorm", flat + PW_KNOBS[1:], e_two, c=32, c_hid=64, **two))
    out.append(_c("gn_16x48_sps2", "mixer", "pytc_pw_wgrad_groupnorm", (), e_two, c=16, c_hid=48, **two))
    out.append(_c("gn_32x64_empty_last_slot", "mixer", "pytc_pw_wgrad_groupnorm", (), ("slots>1", "empty_last", "rows%32", "sps>1"),
                  c=32, c_hid=64, N=1, rows=EMPTY_ROWS))
    return out


def _norm_cases():
    out = []
    small = dict(N=2, rows=347)             # 5 slots per sample of 70 rows, last 67
    e = ("slots>1", "ragged", "rows%32")
    for dt, C in ((BF16, 12), (BF16, 32), (F32, 12), (F32, 32)):
        out.append(_c(f"norm_bwd_{_dtn(dt)}_C{C}", "norm", "pytc_norm_bwd", (), e, dtype=dt, C=C, **small))
        out.append(_c(f"norm_bwd_stats_{_dtn(dt)}_C{C}", "norm", "pytc_norm_bwd_stats", (), e, dtype=dt, C=C, **small))
    out.append(_c("norm_bwd_stats_fp32_C8_empty_slots", "norm", "pytc_norm_bwd_stats", (), ("slots>1", "empty_last", "cap1024", "rows%32"),
                  dtype=F32, C=8, N=1, rows=EMPTY_ROWS))
    out.append(_c("norm_bwd_fp32_C8_cap1024", "norm", "pytc_norm_bwd", (), ("slots>1", "empty_last", "cap1024", "rows%32"),
                  dtype=F32, C=8, N=1, rows=CAP_ROWS))
    # (bf16 C = 8, not 12: pytc_norm_bwd_apply requires rows of whole 16-byte vectors, C % 8 == 0 in bf16)
    for dt, C in ((BF16, 32), (F32, 12), (F32, 32), (BF16, 8)):
        for parts in (1, 3):
            for crop in (0, 1):
                out.append(_c(f"norm_bwd_apply_{_dtn(dt)}_C{C}_parts{parts}" + ("_crop" if crop else ""), "norm", "pytc_norm_bwd_apply", (), e,
                              dtype=dt, C=C, s_parts=parts, crop=crop, N=2, rows=5 * 7 * 11, grid=(5, 7, 11)))      # 385 rows: 6 slots of 65, last 60
    return out


DW_KNOBS = ({"dw_wgrad_march": 0}, {"dw_wgrad_march": 0, "dw_wgrad_vec": 0})


def _dw_cases():
    out = []
    for entry in ("pytc_dw_wgrad", "pytc_dw_wgrad_partial"):
        t = "imm" if entry == "pytc_dw_wgrad" else "part"
        out += [
            # z-march (stride 1, K 3, C % 32 == 0, D >= 8, H, W >= 16) on a grid that is no multiple of its 8 x 8 tiles; the knobs walk
            # the same shape through the vector and the generic form
            _c(f"dw_{t}_march_bf16_C32_9x17x19", "dw", entry, DW_KNOBS, ("slots>1", "rows%32", "march"), dtype=BF16, C=32, K=3, stride=1,
               N=2, gdims=(9, 17, 19), xdims=(9, 17, 19), want_db=1),
            _c(f"dw_{t}_vec_bf16_C16_down_s2", "dw", entry, DW_KNOBS[1:], ("slots>1", "ragged", "rows%32", "vec"), dtype=BF16, C=16, K=3, stride=2,
               N=2, gdims=(5, 11, 13), xdims=(9, 21, 26), want_db=1),
            _c(f"dw_{t}_vec_bf16_C16_up_s2_nodb", "dw", entry, DW_KNOBS[1:], ("slots>1", "ragged", "rows%32", "vec", "transposed"), dtype=BF16, C=16, K=3,
               stride=2, N=2, gdims=(5, 11, 13), xdims=(9, 21, 25), want_db=0),
            _c(f"dw_{t}_vec_fp32_C8_s1", "dw", entry, DW_KNOBS[1:], ("slots>1", "rows%32", "vec"), dtype=F32, C=8, K=3, stride=1,
               N=3, gdims=(5, 6, 7), xdims=(5, 6, 7), want_db=1),
            _c(f"dw_{t}_generic_bf16_C12_k5_s2", "dw", entry, (), ("slots>1", "ragged", "rows%32", "generic"), dtype=BF16, C=12, K=5, stride=2,
               N=2, gdims=(4, 5, 6), xdims=(8, 10, 12), want_db=1),
            _c(f"dw_{t}_generic_bf16_C12_k5_up_s2_nodb", "dw", entry, (), ("slots>1", "ragged", "rows%32", "generic", "transposed"), dtype=BF16, C=12, K=5,
               stride=2, N=2, gdims=(4, 5, 6), xdims=(7, 9, 11), want_db=0),
            _c(f"dw_{t}_generic_fp32_C6_k3_s1", "dw", entry, (), ("slots>1", "rows%32", "generic"), dtype=F32, C=6, K=3, stride=1,
               N=2, gdims=(5, 6, 7), xdims=(5, 6, 7), want_db=1),
        ]
    return out


def _elementwise_cases():
    out = []
    for dt in (BF16, F32):
        d = _dtn(dt)
        out.append(_c(f"gelu_fwd_{d}", "elementwise", "pytc_gelu", (), ("n%vec",), dtype=dt, n=1003, bwd=0))
        out.append(_c(f"gelu_bwd_{d}", "elementwise", "pytc_gelu", (), ("n%vec",), dtype=dt, n=1003, bwd=1))
        out.append(_c(f"gelu_bwd_{d}_multiblock", "elementwise", "pytc_gelu", (), ("n%vec",), dtype=dt, n=16384 * 256 + 5, bwd=1))
        out.append(_c(f"add_inplace_{d}", "elementwise", "pytc_add_inplace", (), ("n%vec",), dtype=dt, n=1003))
        out.append(_c(f"grn_bwd_apply_{d}", "elementwise", "pytc_grn_bwd_apply", (), ("n%vec",), dtype=dt, N=2, rows=37, C=13))
    out.append(_c("copy_zero_front_bf16_C8", "elementwise", "pytc_copy_zero_front", (), (), dtype=BF16, N=2, dims=(3, 4, 5), C=8))
    out.append(_c("copy_zero_front_fp32_C12", "elementwise", "pytc_copy_zero_front", (), (), dtype=F32, N=2, dims=(2, 5, 3), C=12))
    return out


def _dense_cases():
    mf = ({"conv_wgrad_mfma": 0},)
    return [
        _c("conv3d_wgrad_bf16_16x16_k333", "dense", "pytc_conv3d_wgrad", mf, ("mfma",), dtype=BF16, N=2, dims=(4, 11, 13), c_in=16, c_out=16, k=(3, 3, 3)),
        _c("conv3d_wgrad_bf16_24x8_k133", "dense", "pytc_conv3d_wgrad", mf, ("mfma",), dtype=BF16, N=2, dims=(4, 11, 13), c_in=24, c_out=8, k=(1, 3, 3)),
        _c("conv3d_wgrad_fp32_8x12_k333", "dense", "pytc_conv3d_wgrad", (), ("valu",), dtype=F32, N=2, dims=(8, 32, 33), c_in=8, c_out=12, k=(3, 3, 3)),
        _c("conv3d_wgrad_strided_bf16_16x32", "dense", "pytc_conv3d_wgrad_strided", (), ("mfma",), dtype=BF16, N=2, big=(7, 10, 13), c_k=16, c_o=32),
        _c("conv3d_wgrad_strided_fp32_8x8", "dense", "pytc_conv3d_wgrad_strided", (), ("valu",), dtype=F32, N=2, big=(15, 63, 65), c_k=8, c_o=8),
        _c("upcat_deconv2_wgrad_bf16_16to8_e8_odd", "dense", "pytc_upcat_deconv2_wgrad", (), (), dtype=BF16, N=2, lo=(3, 5, 6), sk=(7, 10, 13), c_in=16, c_u=8, c_e=8),
        _c("upcat_deconv2_wgrad_fp32_8to8_e4", "dense", "pytc_upcat_deconv2_wgrad", (), (), dtype=F32, N=1, lo=(3, 5, 6), sk=(6, 11, 12), c_in=8, c_u=8, c_e=4),
        _c("deconv2_upfirst_wgrad_bf16_32to16_e16", "dense", "pytc_deconv2_upfirst_wgrad", (), (), dtype=BF16, N=2, lo=(3, 5, 6), c_in=32, c_u=16, c_e=16),
        _c("deconv2_upfirst_wgrad_bf16_16to8_e0", "dense", "pytc_deconv2_upfirst_wgrad", (), (), dtype=BF16, N=1, lo=(3, 5, 7), c_in=16, c_u=8, c_e=0),
    ]


@functools.lru_cache(maxsize=None)
def cases():
    out = _pw_cases() + _mixer_cases() + _norm_cases() + _dw_cases() + _elementwise_cases() + _dense_cases()
    assert len({c.id for c in out}) == len(out), "duplicate case id"
    return tuple(out)


FAMILIES = ("pw", "mixer", "norm", "dw", "elementwise", "dense")


def by_family(fam):
    return [c for c in cases() if c.family == fam]


def table_entries():
    return sorted({c.entry for c in cases()} | {REDUCE_ENTRY})


# ------------------------------------------------------------------------------------------------------------------ slot facts
def launch_slots(c: Case, knobs=None) -> int | None:
    """Slots the launch writes (*slots_out), by the mirrors of exact_reduction_cases.py; None where no mirror exists."""
    kn = dict(knobs or ())
    p = dict(c.p)
    if c.family == "pw":
        total = p["N"] * p["rows"]
        # (wgrad_valu changes the kernel, not the split: bf16 with 16-channel tiles keeps the matrix-core slot count)
        mk = dict(whole_rounds=bool(kn.get("wgrad_whole_rounds", 1)), small_split=bool(kn.get("wgrad_small_split", 1)))
        return X.pw_launch_slots(total, p["c_in"], p["c_out"], bf16=p["dtype"] == BF16, **mk)
    if c.entry == "pytc_mixer_bwd_rc":
        return p["N"] * X.mixer_bwd_rc_sps(p["N"], p["rows"], p["c_hid"], slot_div=kn.get("mixer_bwd_rc_slot_div", 1))
    if c.entry == "pytc_pw_wgrad_groupnorm":
        if "wgrad_small_split" in kn or "wgrad_whole_rounds" in kn:
            mk = dict(whole_rounds=bool(kn.get("wgrad_whole_rounds", 1)), small_split=bool(kn.get("wgrad_small_split", 1)))
            return p["N"] * max(1, X.wgrad_mfma_slots(p["N"] * p["rows"], p["c"], p["c_hid"], **mk) // p["N"])
        return p["N"] * X.pw_wgrad_groupnorm_sps(p["N"], p["rows"], p["c"], p["c_hid"])
    if c.family == "norm":
        return X.colstats_slots(p["rows"])                       # per sample
    if c.family == "dw" and p["dtype"] == BF16:                  # (the mirror restates the bf16 vector widths)
        return X.dw_wgrad_slots(p["N"], p["gdims"], p["xdims"], p["C"], p["K"], p["stride"], march=bool(kn.get("dw_wgrad_march", 1)),
                                vec=bool(kn.get("dw_wgrad_vec", 1)))
    return None


def dw_form(c: Case, knobs=None) -> str:
    kn = dict(knobs or ())
    p = dict(c.p)
    if p["dtype"] != BF16:                                       # fp32: 4 elements per 16 bytes, no z-march
        return "vec" if kn.get("dw_wgrad_vec", 1) and p["K"] == 3 and p["C"] % 4 == 0 and p["C"] // 4 <= 256 else "generic"
    return X.dw_wgrad_form(p["gdims"], p["xdims"], p["C"], p["K"], p["stride"], march=bool(kn.get("dw_wgrad_march", 1)),
                           vec=bool(kn.get("dw_wgrad_vec", 1)))


def slot_facts(c: Case) -> dict:
    """What the mirrors say about the case's row split: slots, rows per slot, ragged last slot, a slot / a 32-row block across a sample
    boundary, empty slots."""
    p = dict(c.p)
    s = launch_slots(c)
    if c.family == "pw":
        total, per = p["N"] * p["rows"], p["rows"]
        n_split = 1
    elif c.family in ("mixer", "norm"):
        total, per, n_split = p["rows"], p["rows"], p["N"]       # slots split one sample's rows
        s = s // p["N"] if c.family == "mixer" else s
    else:
        return dict(slots=s)
    rps = -(-total // s)
    used = -(-total // rps)
    last = total - (used - 1) * rps
    straddle = n_split == 1 and p["N"] > 1 and any((a // per) != ((min(a + rps, total) - 1) // per) for a in range(0, total, rps))
    block32 = p["N"] > 1 and per % 32 != 0
    return dict(slots=s * n_split, per_split=s, rows_per_slot=rps, used=used, empty=s - used, ragged=last != rps, straddle=straddle,
                block32_straddle=block32 and n_split == 1)


# ------------------------------------------------------------------------------------------------------------------ references
def _cap_gemm(a64, b64, quantum, what):
    """sum_r |a_rk| |b_ro| of every output of a^T b stays an exact fp32 integer count of `quantum`"""
    X.assert_exact_cap(X.gemm_abs_bound(float(a64.abs().max()), b64.abs().sum(0)), quantum, what=what)


def conv_wgrad_ref(small, big, kernel, stride, pad, depthwise=False):
    """fp64 sum_r small[r][o] * big[r * stride + tap - pad][k] (zeros outside big) -> [taps][C_o][C_k], or [taps][C] depthwise."""
    N, d, h, w, co = small.shape
    ck = big.shape[-1]
    dims = (d, h, w)
    lp = [int(v) for v in pad]
    rp = [max(0, stride[i] * (dims[i] - 1) + kernel[i] - lp[i] - big.shape[1 + i]) for i in range(3)]
    bp = F.pad(big.double(), (0, 0, lp[2], rp[2], lp[1], rp[1], lp[0], rp[0]))
    s = small.double().reshape(-1, co)
    out = []
    for kz in range(kernel[0]):
        for ky in range(kernel[1]):
            for kx in range(kernel[2]):
                sl = bp[:, kz:kz + stride[0] * (d - 1) + 1:stride[0], ky:ky + stride[1] * (h - 1) + 1:stride[1],
                        kx:kx + stride[2] * (w - 1) + 1:stride[2]].reshape(-1, ck)
                out.append((s * sl).sum(0) if depthwise else s.t() @ sl)
    return torch.stack(out)


def _seed(c: Case) -> int:
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(c.id)) % 100003


def _build_pw(c):
    p, seed = dict(c.p), _seed(c)
    N, rows, ci, co, dt = p["N"], p["rows"], p["c_in"], p["c_out"], p["dtype"]
    if p["gelu"]:
        x = X.binary((N, rows, ci), 0.5, seed, value=16.0, dtype=dt)         # gelu(0) = 0, gelu(16) = 16 under every form
    else:
        x = X.ternary((N, rows, ci), 0.5, seed, dtype=dt)
    xn = x.double()
    inputs = {"x": x}
    quantum = 16.0 if p["gelu"] else 1.0
    if p["ab"]:
        ab = X.exact_affine(N, ci, seed + 7)
        inputs["ab"] = ab
        xn = xn * ab[:, 0].double()[:, None] + ab[:, 1].double()[:, None]
        quantum = 0.5
        assert X.is_bf16_exact(xn)                                          # the kernels round a x + b to the storage type
    dy = X.ternary((N, rows, co), 0.25, seed + 1, dtype=dt)
    inputs["dy"] = dy
    dyd = dy.double().reshape(-1, co)
    _cap_gemm(xn, dyd, quantum, c.id)
    X.assert_exact_cap(float(dyd.abs().sum(0).max()), 1.0, what=c.id + " db")
    dW = dyd.t() @ xn.reshape(-1, ci)
    db = dyd.sum(0)
    b = Built(inputs, {}, {"dW": dW.reshape(-1), "db": db})
    if c.entry == "pytc_pw_wgrad":
        b.outputs["dW"] = Ref(F32, dW)
        if p["want_db"]:
            b.outputs["db"] = Ref(F32, db)
    if c.entry == "pytc_pw_wgrad_dgrad_partial":
        w = X.ternary((co, ci), 0.5, 11, dtype=F32)
        inputs["w"] = w
        dx = (dyd @ w.double()).view(N, rows, ci) * torch.where(x.double() == 16.0, 1.0, 0.5)   # gelu'(0) = 1/2, gelu'(16) = 1
        assert float(dx.abs().max()) <= co and X.is_bf16_exact(dx)
        b.outputs["dx"] = Ref(BF16, dx)
    return b


def pw_regions(c, slots):
    p = dict(c.p)
    nW, nB = p["c_in"] * p["c_out"], p["c_out"]
    return [Region("dW", 0, slots, nW, None), Region("db", slots * nW, slots, nB, None, written=bool(p["want_db"]))]


def mixer_operands(N, rows, C, c_hid, seed):
    """t in {0, 1}; affine a t + b in {(16, 0), (-16, 16)} per channel -> {0, 16}; exact statistics with rstd per channel, mean per
    (sample, channel): gamma = a / rstd, beta = b + mean a; W2 one-hot (hp[h] = xn[h mod C]), b2 = 0; W3 ternary"""
    t = X.binary((N, rows, C), 0.5, seed, value=1.0)
    g = torch.Generator().manual_seed(seed + 1)
    neg = (torch.rand(C, generator=g) < 0.5).expand(N, C)
    ab = torch.stack([torch.where(neg, -16.0, 16.0), torch.where(neg, 16.0, 0.0)], 1).contiguous()
    rstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)].expand(N, C)
    mean = torch.randint(-1, 2, (N, C), generator=g).float()
    mr = torch.stack([mean, rstd], 1).contiguous()
    gamma = (ab[0, 0] / rstd[0]).contiguous()
    w2 = torch.zeros((c_hid, C), dtype=F32)
    w2[torch.arange(c_hid), torch.arange(c_hid) % C] = 1.0
    w3 = X.ternary((32, c_hid), 0.5, seed + 2, dtype=F32)
    dy = X.ternary((N, rows, 32), 0.5, seed + 3)
    return t, ab, mr, gamma, w2, w3, dy


def _norm_coef(s, mr, gamma, count):
    """coef [N][3][C] = (A, B, C) with dt = A dtn + B t + C the GroupNorm backward (fp64)"""
    mean, rstd = mr[:, 0].double(), mr[:, 1].double()
    rg = rstd * gamma.double()
    m1, m2 = s[:, 0] / count, s[:, 1] / count
    B = -rg * rstd * m2
    return torch.stack([rg, B, -rg * m1 - B * mean], 1)


def _is_f32_exact(t64):
    return bool(torch.equal(t64.float().double(), t64))


def _build_mixer(c):
    p, seed = dict(c.p), _seed(c)
    N, rows = p["N"], p["rows"]
    if c.entry == "pytc_mixer_bwd_rc":
        C, hid, gn = 32, p["c_hid"], p["gn"]
        t, ab, mr, gamma, w2, w3, dy = mixer_operands(N, rows, C, hid, seed)
        xn = t.double() * ab[:, 0].double()[:, None] + ab[:, 1].double()[:, None]
        hp = xn[..., torch.arange(hid) % C]
        assert set(hp.unique().tolist()) <= {0.0, 16.0}
        dyd = dy.double().reshape(-1, 32)
        _cap_gemm(hp, dyd, 16.0, c.id)
        dhp = (dyd @ w3.double()).view(N, rows, hid) * torch.where(hp == 16, 1.0, 0.5)
        assert X.is_bf16_exact(dhp)
        inputs = {"t": t, "ab": ab, "dy": dy, "w2": w2, "b2": torch.zeros(hid), "w3": w3}
        b = Built(inputs, {"dhp": Ref(BF16, dhp)}, {"dW3": (dyd.t() @ hp.reshape(-1, hid)).reshape(-1), "db3": dyd.sum(0)})
        count = 1024.0
    else:
        C, hid, gn = p["c"], p["c_hid"], 1
        t = X.ternary((N, rows, C), 0.5, seed)
        g = torch.Generator().manual_seed(seed + 1)
        mean = torch.randint(-1, 2, (N, C), generator=g).float()
        rstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (N, C), generator=g)]
        gamma = torch.tensor([1.0, -1.0, 2.0, -2.0])[torch.randint(0, 4, (C,), generator=g)]
        beta = torch.randint(-1, 2, (C,), generator=g).float()
        a = gamma * rstd
        ab = torch.stack([a, beta - mean * a], 1).contiguous()
        mr = torch.stack([mean, rstd], 1).contiguous()
        dhp_in = X.ternary((N, rows, hid), 1.0 / 16, seed + 2)
        w2 = X.ternary((hid, C), 0.5, seed + 3, dtype=F32)
        dhp = dhp_in.double()
        xn = ((t.double() - mean.double()[:, None]) * rstd.double()[:, None]) * gamma.double() + beta.double()
        inputs = {"t": t, "mr": mr, "ab": ab, "dhp": dhp_in, "w2": w2, "gamma": gamma}
        b = Built(inputs, {}, {})
        count = 2048.0
    if gn:
        xhat = (t.double() - mr[:, 0].double()[:, None]) * mr[:, 1].double()[:, None]
        assert X.is_bf16_exact(xhat)                                          # the high / low split of the operand loses nothing
        dh = dhp.reshape(N, rows, hid)
        _cap_gemm(xn, dh.reshape(-1, hid), 1.0 / 8, c.id + " dW2")
        _cap_gemm(xhat, dh.reshape(-1, hid), 1.0 / 8, c.id + " M")
        M = torch.einsum("nrh,nrc->nhc", dh, xhat)
        q = dh.sum(1)
        w2b = w2.double()
        assert X.is_bf16_exact(w2b)
        s = torch.stack([torch.einsum("hc,nh->nc", w2b, q), torch.einsum("hc,nhc->nc", w2b, M)], 1)
        coef = _norm_coef(s, mr, gamma, count)
        assert _is_f32_exact(s) and _is_f32_exact(coef) and float(s.abs().max()) < X.EXACT_F32 / 16
        inputs.update(mr=mr, gamma=gamma)
        b.inputs["count"] = count
        b.outputs["s_out"] = Ref(F32, s)
        b.outputs["coef"] = Ref(F32, coef)
        b.totals.update(M=M.sum(0).reshape(-1), q=q.sum(0), dW2=(dh.reshape(-1, hid).t() @ xn.reshape(-1, C)).reshape(-1), db2=q.sum(0))
    return b


def mixer_regions(c, slots):
    """pytc_mixer_bwd_rc: dW3 partials [S][32][C_hid] | db3 partials [S][32] | gn: M partials [S][C_hid][32] | q partials [S][C_hid] |
    term [N][C_hid][32] | q [N][C_hid]"""
    p = dict(c.p)
    hid, N, S = p["c_hid"], p["N"], slots
    per = 32 * hid
    out = [Region("dW3", 0, S, per, None), Region("db3", S * per, S, 32, None, written=bool(p["want_db3"]))]
    if p["gn"]:
        o = S * (per + 32)
        out += [Region("M", o, S, per, None), Region("q", o + S * per, S, hid, None), Region("dW2", o + S * (per + hid), N, per, None),
                Region("db2", o + S * (per + hid) + N * per, N, hid, None)]
    return out


def groupnorm_regions(c, slots):
    """pytc_pw_wgrad_groupnorm: [N sps][C_hid C] dW partials | [N sps][C_hid] bias partials | term [N][C_hid C] | q [N][C_hid]; with
    sps == 1 the samples' terms are left in the dW partials region and `term` is not written"""
    p = dict(c.p)
    N, nW, hid = p["N"], p["c"] * p["c_hid"], p["c_hid"]
    S = slots
    if S == N:
        return [Region("dW2", 0, N, nW, None), Region("q", N * nW, N, hid, None), Region("term_unused", N * (nW + hid), N, nW, None, written=False),
                Region("db2", N * (nW + hid) + N * nW, N, hid, None)]
    return [Region("M", 0, S, nW, None), Region("q", S * nW, S, hid, None), Region("dW2", S * (nW + hid), N, nW, None),
            Region("db2", S * (nW + hid) + N * nW, N, hid, None)]


def _norm_stats_operands(N, rows, C, dt, seed):
    g = torch.Generator().manual_seed(seed + 5)
    dtn = X.ternary((N, rows, C), 0.5, seed, dtype=dt)
    t = X.ternary((N, rows, C), 0.5, seed + 1, dtype=dt)
    mean = torch.randint(-1, 2, (N, C), generator=g).float()
    rstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (N, C), generator=g)]
    gamma = torch.tensor([1.0, -1.0, 2.0, -2.0])[torch.randint(0, 4, (C,), generator=g)]
    return dtn, t, torch.stack([mean, rstd], 1).contiguous(), gamma


def _build_norm(c):
    p, seed = dict(c.p), _seed(c)
    N, rows, C, dt = p["N"], p["rows"], p["C"], p["dtype"]
    dtn, t, mr, gamma = _norm_stats_operands(N, rows, C, dt, seed)
    xhat = (t.double() - mr[:, 0].double()[:, None]) * mr[:, 1].double()[:, None]
    d = dtn.double()
    rg = (mr[:, 1].double() * gamma.double())[:, None]
    inputs = {"dtn": dtn, "t": t, "mr": mr, "gamma": gamma}
    if c.entry == "pytc_norm_bwd_apply":
        parts, count = p["s_parts"], 256.0
        g = torch.Generator().manual_seed(seed + 9)
        vals = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0]) * count
        s_parts = vals[torch.randint(0, 5, (parts, N, 2, C), generator=g)] * (1.0 if parts == 1 else 0.25)      # three parts: |sum| <= 3/4 count
        s = s_parts.double().sum(0)
        assert _is_f32_exact(s)
        dt_ref = rg * (d - s[:, 0][:, None] / count - xhat * s[:, 1][:, None] / count)
        if dt == BF16:
            assert X.is_bf16_exact(dt_ref), c.id
        assert _is_f32_exact(dt_ref)
        if p["crop"]:
            D, H, W = p["grid"]
            dt_ref = dt_ref.view(N, D, H, W, C)[:, 1:, 1:, 1:].reshape(N, -1, C)
        inputs.update(s_in=s_parts.contiguous(), count=count)
        return Built(inputs, {"dt": Ref(dt, dt_ref)})
    X.assert_exact_cap(rows * 4.0, 0.5, what=c.id)                           # |dtn xhat| <= 4, quantum 1/2
    s = torch.stack([d.sum(1), (d * xhat).sum(1)], 1)
    outs = {"s_out": Ref(F32, s)}
    count = 512.0
    if c.entry == "pytc_norm_bwd":
        dt_ref = rg * (d - s[:, 0][:, None] / count - xhat * s[:, 1][:, None] / count)
        assert _is_f32_exact(dt_ref), c.id                                   # the value before the store is exact in fp32
        outs["dt"] = Ref(dt, dt_ref, ulp=0 if dt == F32 else 1)
        inputs["count"] = count
    return Built(inputs, outs, {"stats": s.reshape(N, -1)})


def _build_dw(c):
    p, seed = dict(c.p), _seed(c)
    N, C, K, st, dt = p["N"], p["C"], p["K"], p["stride"], p["dtype"]
    g = X.ternary((N, *p["gdims"], C), 0.5, seed, dtype=dt)
    x = X.ternary((N, *p["xdims"], C), 0.5, seed + 1, dtype=dt)
    X.assert_exact_cap(N * p["gdims"][0] * p["gdims"][1] * p["gdims"][2], 1.0, what=c.id)
    dW = conv_wgrad_ref(g, x, (K,) * 3, (st,) * 3, (K // 2,) * 3, depthwise=True)          # [K^3][C]
    db = g.double().reshape(-1, C).sum(0)
    b = Built({"g": g, "x": x}, {}, {"dW": dW.reshape(-1), "db": db})
    if c.entry == "pytc_dw_wgrad":
        b.outputs["dW"] = Ref(F32, dW)
        if p["want_db"]:
            b.outputs["db"] = Ref(F32, db)
    return b


def dw_regions(c, slots):
    p = dict(c.p)
    nW, nB = p["K"] ** 3 * p["C"], p["C"]
    return [Region("dW", 0, slots, nW, None), Region("db", slots * nW, slots, nB, None, written=bool(p["want_db"]))]


def _build_elementwise(c):
    p, seed = dict(c.p), _seed(c)
    dt = p["dtype"]
    if c.entry == "pytc_gelu":
        x = X.binary((p["n"],), 0.5, seed, value=16.0, dtype=dt)
        if not p["bwd"]:
            return Built({"x": x}, {"out": Ref(dt, x.double())})                               # gelu(0) = 0, gelu(16) = 16
        dy = X.ternary((p["n"],), 0.75, seed + 1, scale=2.0, dtype=dt)
        return Built({"x": x, "dy": dy}, {"out": Ref(dt, dy.double() * torch.where(x.double() == 16.0, 1.0, 0.5))})
    if c.entry == "pytc_add_inplace":
        y0 = X.ternary((p["n"],), 0.75, seed, scale=4.0, dtype=dt)
        x = X.ternary((p["n"],), 0.75, seed + 1, dtype=dt)
        return Built({"x": x}, {"y": Ref(dt, y0.double() + x.double())}, inout={"y": y0})
    if c.entry == "pytc_copy_zero_front":
        N, (D, H, W), C = p["N"], p["dims"], p["C"]
        src = X.ternary((N, D, H, W, C), 0.9, seed, dtype=dt)
        ref = src.double().clone()
        ref[:, 0] = 0; ref[:, :, 0] = 0; ref[:, :, :, 0] = 0
        return Built({"src": src}, {"dst": Ref(dt, ref)})
    N, rows, C = p["N"], p["rows"], p["C"]                                   # grn_bwd_apply
    g = torch.Generator().manual_seed(seed + 3)
    dh2 = X.ternary((N, rows, C), 0.75, seed, dtype=dt)
    hp = X.binary((N, rows, C), 0.5, seed + 1, value=16.0, dtype=dt)
    A = torch.tensor([1.0, -1.0, 2.0, 0.5])[torch.randint(0, 4, (N, C), generator=g)]
    B = torch.tensor([0.0, 0.125, -0.125, 0.25])[torch.randint(0, 4, (N, C), generator=g)]
    ref = (dh2.double() * A.double()[:, None] + hp.double() * B.double()[:, None]) * torch.where(hp.double() == 16.0, 1.0, 0.5)
    assert X.is_bf16_exact(ref)
    return Built({"dh2": dh2, "hp": hp, "A": A, "B": B}, {"out": Ref(dt, ref)})


def fold_replicate(d_up, lo_dims):
    """gradient of replicate-padding a (2 lo)-grid to the skip's grid: an extra last plane folds into the plane before it"""
    for ax in range(3):
        n2 = 2 * lo_dims[ax]
        if d_up.shape[1 + ax] == n2 + 1:
            last = d_up.narrow(1 + ax, n2, 1)
            d_up = d_up.narrow(1 + ax, 0, n2).clone()
            d_up.narrow(1 + ax, n2 - 1, 1).add_(last)
    return d_up


def _build_dense(c):
    p, seed = dict(c.p), _seed(c)
    dt, N = p["dtype"], p["N"]
    if c.entry == "pytc_conv3d_wgrad":
        a = X.ternary((N, *p["dims"], p["c_in"]), 0.5, seed, dtype=dt)
        dy = X.ternary((N, *p["dims"], p["c_out"]), 0.5, seed + 1, dtype=dt)
        X.assert_exact_cap(a[..., 0].numel(), 1.0, what=c.id)
        return Built({"a": a, "dy": dy}, {"dW": Ref(F32, conv_wgrad_ref(dy, a, p["k"], (1, 1, 1), tuple(v // 2 for v in p["k"])))})
    if c.entry == "pytc_conv3d_wgrad_strided":
        small = tuple((v + 1) // 2 for v in p["big"])
        big = X.ternary((N, *p["big"], p["c_k"]), 0.5, seed, dtype=dt)
        sm = X.ternary((N, *small, p["c_o"]), 0.5, seed + 1, dtype=dt)
        X.assert_exact_cap(sm[..., 0].numel(), 1.0, what=c.id)
        return Built({"big": big, "small": sm}, {"dW": Ref(F32, conv_wgrad_ref(sm, big, (3, 3, 3), (2, 2, 2), (1, 1, 1)))})
    lo, ci, cu, ce = p["lo"], p["c_in"], p["c_u"], p["c_e"]
    x_low = X.ternary((N, *lo, ci), 0.5, seed, dtype=dt)
    hi = p["sk"] if c.entry == "pytc_upcat_deconv2_wgrad" else tuple(2 * v for v in lo)
    d = X.ternary((N, *hi, ce + cu), 0.5, seed + 1, dtype=dt)
    up = d[..., ce:] if c.entry == "pytc_upcat_deconv2_wgrad" else d[..., :cu]
    X.assert_exact_cap(8.0 * x_low[..., 0].numel(), 1.0, what=c.id)           # a folded plane doubles a term per axis
    taps = conv_wgrad_ref(x_low, fold_replicate(up.double(), lo), (2, 2, 2), (2, 2, 2), (0, 0, 0))       # [8][C_in][C_u]
    dw = taps.permute(1, 2, 0).reshape(ci, cu, 2, 2, 2)
    return Built({"x_low": x_low, "d": d}, {"dw": Ref(F32, dw), "db": Ref(F32, up.double().reshape(-1, cu).sum(0))})


_BUILDERS = {"pw": _build_pw, "mixer": _build_mixer, "norm": _build_norm, "dw": _build_dw, "elementwise": _build_elementwise,
             "dense": _build_dense}


@functools.lru_cache(maxsize=None)
def _build_cached(c: Case) -> Built:
    b = _BUILDERS[c.family](c)
    for name, r in b.outputs.items():                                        # every reference is a number of its storage type
        if r.ulp == 0:
            ok = X.is_bf16_exact(r.ref) if r.dtype == BF16 else _is_f32_exact(r.ref)
            assert ok, f"{c.id}: the reference of {name} is not exact in {r.dtype}"
    return b


def build(c: Case) -> Built:
    """Operands and references of a case, computed once per process and shared (callers must not modify them)."""
    return _build_cached(c)


def regions(c: Case, slots: int):
    """The documented slot-partial regions of the case's workspace for *slots_out = slots, with the fp64 totals filled in."""
    fn = {"pytc_pw_wgrad_partial": pw_regions, "pytc_pw_wgrad_dgrad_partial": pw_regions, "pytc_dw_wgrad_partial": dw_regions,
          "pytc_mixer_bwd_rc": mixer_regions, "pytc_pw_wgrad_groupnorm": groupnorm_regions}.get(c.entry)
    if fn is None:
        return []
    tot = build(c).totals
    out = fn(c, slots)
    for r in out:
        r.total = tot.get(r.name)
    return out


def ulp_distance(got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """units in the last place between two finite tensors of one 16- or 32-bit float type (by their ordered bit patterns)"""
    it = torch.int16 if got.element_size() == 2 else torch.int32
    def key(t):
        b = t.contiguous().view(it).to(torch.int64)
        return torch.where(b < 0, -(b & (0x7FFF if it == torch.int16 else 0x7FFFFFFF)), b)
    return (key(got) - key(want)).abs()

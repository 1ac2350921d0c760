"""CPU checks of the label-target work: the gather-form numpy model against the fixture recorded from the reference's functions, the
planner of data/label_targets.py (layout, names, defaults, every error and refusal), and the training module's `label_mask` handling
on CPU tensors with a stand-in model, as tests/test_host_training_module.py does."""
import sys
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import label_target_cases as LC  # noqa: E402
from loss_cases import loss_cfg  # noqa: E402

from pytorch_connectomics_amd import _native as nat  # noqa: E402
from pytorch_connectomics_amd.data import LabelTargetTransform, device_target_batches, labels_to_int32  # noqa: E402
from pytorch_connectomics_amd.training.module import (ConnectomicsModule, check_label_mask, fit,  # noqa: E402
                                                      resize_label_mask_to_output, validate, weighted_bce_with_logits)

GOLD = Path(__file__).resolve().parent / "golden" / "label_targets.npz"


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLD))


# ---------------------------------------------------------------------------------------------------------------- model == fixture
@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_numpy_model_equals_the_reference_fixture(name, golden):
    case = LC.CASES[name]
    label = LC.make_label(name)
    assert label.dtype == np.int32 and np.array_equal(label, golden[f"{name}__label"])
    assert (label == -1).any() and (label == 0).any() and (label > 0).any()
    for half in case["erode"]:
        got = np.stack([LC.model_erode(s, half) for s in label])
        assert np.array_equal(got, golden[f"{name}__erode_{half[0]}_{half[1]}_{half[2]}"]), (name, half)
    for k, cfg in enumerate(case["configs"]):
        values, mask = LC.model_batch(label, cfg)
        assert values.dtype == np.float32 and np.array_equal(values, golden[f"{name}__{k}__values"].astype(np.float32)), (name, k)
        if mask is None:
            assert f"{name}__{k}__mask" not in golden
        else:
            assert np.array_equal(mask, golden[f"{name}__{k}__mask"]), (name, k)
        plan = LabelTargetTransform.from_config(cfg)
        assert plan.channels == values.shape[1] and plan.uses_mask == (mask is not None)


def test_fixture_covers_what_the_cases_claim(golden):
    v = golden["banis_long_range__0__values"]
    assert not v[:, 4].any() and not golden["banis_long_range__0__mask"][:, 4].any() and v[:, 3].any() and v[:, 5].any()
    d1 = golden["depth1__0__values"]
    assert not d1[:, 0].any() and not golden["depth1__0__mask"][:, 0].any() and d1[:, 1].any()
    assert set(np.unique(golden["no_affinity__0__values"][:, 10])) == {0, 1, 2}
    ids = set(np.unique(golden["big_ids__label"]).tolist())
    assert {1, 1 + 2 ** 24, 2 ** 31 - 1} <= ids
    for half in ((10, 10, 4),):                              # a half-size larger than an axis is a window clipped to the whole axis
        assert golden[f"aff12_erosion1__erode_{half[0]}_{half[1]}_{half[2]}"].shape == (2, 5, 31, 33)


# ---------------------------------------------------------------------------------------------------------------- the planner
def test_planner_layout_names_and_defaults():
    plan = LabelTargetTransform.from_config(NS(erosion=1, stack_outputs=True, output_dtype="float32", targets=[
        {"name": "affinity", "kwargs": {"affinity_mode": "DeepEM ", "erosion": 2}},
        "binary",
        {"task": "instance_boundary"},
        {"type": "polarity"},
        {"name": "polarity", "kwargs": {"exclusive": True}},
        {"name": "eroded_foreground"},
        {"name": "eroded_foreground", "kwargs": {"tsz_h": [2, 2, 1]}},
        {"name": "affinity", "kwargs": {"affinity_mode": "deepem", "long_range": 7, "offsets": ["9-9-9"]}},
        {"name": "binary", "kwargs": {"segment_id": [3, 5], "erosion": 2}}]))
    assert plan.channels == 3 + 1 + 1 + 3 + 1 + 1 + 1 + 6 + 1 == len(plan.channel_names) and plan.uses_mask
    assert plan.affinity_mode == "deepem" and plan.global_erosion == 1
    assert plan.channel_names[:5] == ["affinity[1,0,0]", "affinity[0,1,0]", "affinity[0,0,1]", "binary", "instance_boundary"]
    assert plan.channel_names[5:9] == ["polarity.pos", "polarity.neg", "polarity.fg", "polarity"]
    assert plan.channel_names[11:17] == [f"affinity[{a},{b},{c}]" for a, b, c in
                                         ((1, 0, 0), (0, 1, 0), (0, 0, 1), (7, 0, 0), (0, 7, 0), (0, 0, 7))]      # long_range wins
    g, e2 = (0, 1, 1), (0, 2, 2)
    # the global erosion comes first; distinct erosions share buffers (affinity, the default eroded_foreground and the last binary
    # all read the patch eroded by 1 and then by 2)
    assert plan.sources == [(g, e2), (g,), (g, (2, 2, 1))]
    rows = plan.describe()
    assert [r["chain"] for r in rows[:3]] == [(g, e2)] * 3 and rows[3]["chain"] == (g,) and rows[9]["chain"] == (g, e2)
    assert rows[10]["chain"] == (g, (2, 2, 1)) and rows[17]["chain"] == (g, e2) and rows[17]["v"] == [3, 5]
    assert rows[4]["flags"] == nat.LABEL_EDGE_MODES["seg-all"] and rows[4]["kind"] == nat.LABEL_BOUNDARY      # thickness 1, seg-all, 3d
    t = plan.table
    assert [t[i].source for i in range(plan.channels)] == [0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 2, 1, 1, 1, 1, 1, 1, 0]
    assert (t[17].kind, t[17].n_ids, t[17].v[0], t[17].v[1]) == (nat.LABEL_BINARY, 2, 3, 5)
    assert (t[14].kind, t[14].v[0], t[14].v[1], t[14].v[2]) == (nat.LABEL_AFFINITY, 7, 0, 0)
    # negative offsets as lists; banis and semantic flags; a scalar tsz_h is in-plane
    p2 = LabelTargetTransform.from_config({"targets": [
        {"name": "affinity", "kwargs": {"affinity_mode": "banis", "offsets": [[-1, 2, 0], (0, 0, -5)]}},
        {"name": "affinity", "kwargs": {"affinity_mode": "banis", "semantic": True}},
        {"name": "instance_boundary", "kwargs": {"mode": "2d", "edge_mode": "seg-no-bg"}},
        {"name": "eroded_foreground", "kwargs": {"tsz_h": 3}}]})
    assert p2.channel_names[:2] == ["affinity[-1,2,0]", "affinity[0,0,-5]"] and p2.global_erosion == 0
    assert p2.table[0].flags == nat.LABEL_FLAG_BANIS and p2.table[2].flags == nat.LABEL_FLAG_BANIS | nat.LABEL_FLAG_SEMANTIC
    assert [p2.table[0].v[i] for i in range(3)] == [-1, 2, 0]
    assert p2.table[5].flags == nat.LABEL_EDGE_MODES["seg-no-bg"] | nat.LABEL_FLAG_2D
    assert p2.sources == [(), ((0, 3, 3),)]
    # no affinity: no mask
    p3 = LabelTargetTransform.from_config({"targets": "binary"})
    assert p3.channels == 1 and not p3.uses_mask and p3.affinity_mode is None and p3.sources == [()]


def test_planner_keeps_the_reference_errors():
    mk = LabelTargetTransform.from_config
    with pytest.raises(ValueError, match="Affinity target requires kwargs.affinity_mode: 'deepem' or 'banis'."):
        mk({"targets": ["affinity"]})
    with pytest.raises(ValueError, match="Unsupported affinity_mode 'both'. Expected one of: deepem, banis."):
        mk({"targets": [LC._aff(affinity_mode="both")]})
    with pytest.raises(KeyError) as e:
        mk({"targets": ["binary", "watershed"]})
    assert "Unknown task 'watershed'. Available: affinity, binary, decode_quantize, energy_quantize, eroded_foreground, flow, " \
           "instance_boundary, instance_edt, lsd, polarity, sdt, semantic_edt, signed_distance, skeleton_aware_edt, small_object, " \
           "thin_affinity_weight" in str(e.value)
    with pytest.raises(ValueError, match="Invalid affinity offset '1-0'. Expected 'z-y-x' format."):
        mk({"targets": [LC._aff(affinity_mode="deepem", offsets=["1-0"])]})
    with pytest.raises(ValueError, match="Invalid affinity offset '0-0--5'"):          # the string form cannot say a negative offset
        mk({"targets": [LC._aff(affinity_mode="deepem", offsets=["0-0--5"])]})
    with pytest.raises(ValueError, match="Unsupported affinity offset \\[1, 2\\]. Expected 'z-y-x' string or length-3 sequence."):
        mk({"targets": [LC._aff(affinity_mode="deepem", offsets=[[1, 2]])]})
    with pytest.raises(ValueError, match="semantic=True supports unit offsets only; got \\['0-0-3', '1-1-0'\\]"):
        mk({"targets": [LC._aff(affinity_mode="deepem", semantic=True, offsets=["0-0-1", "0-0-3", "1-1-0"])]})
    with pytest.raises(ValueError, match="Mixed affinity_mode values are not supported in one label stack: \\['banis', 'deepem'\\]"):
        mk({"targets": [LC._aff(affinity_mode="deepem"), LC._aff(affinity_mode="banis")]})
    with pytest.raises(ValueError, match="missing 'name'/'task'/'type'"):
        mk({"targets": [{"kwargs": {}}]})
    with pytest.raises(TypeError, match="Unsupported task specification: 3"):
        mk({"targets": [3]})
    with pytest.raises(ValueError, match="At least one task must be specified"):
        mk({"targets": []})
    with pytest.raises(ValueError, match="tsz_h sequence length 2 != seg ndim 3"):
        mk({"targets": [{"name": "eroded_foreground", "kwargs": {"tsz_h": [2, 2]}}]})
    with pytest.raises(TypeError, match="unexpected kwargs \\['radius'\\]"):
        mk({"targets": [{"name": "binary", "kwargs": {"radius": 2}}]})


@pytest.mark.parametrize("task", ["instance_edt", "semantic_edt", "signed_distance", "sdt", "skeleton_aware_edt", "flow", "lsd",
                                  "small_object", "thin_affinity_weight", "energy_quantize", "decode_quantize"])
def test_planner_refuses_the_unbuilt_targets_by_name(task):
    with pytest.raises(NotImplementedError, match=f"'{task}'"):
        LabelTargetTransform.from_config({"targets": ["binary", {"name": task, "kwargs": {"sigma": 80}}]})


def test_planner_refuses_what_the_kernels_do_not_cover():
    mk = LabelTargetTransform.from_config
    with pytest.raises(NotImplementedError, match="'instance_boundary' with thickness 2"):
        mk({"targets": [{"name": "instance_boundary", "kwargs": {"thickness": 2}}]})
    with pytest.raises(NotImplementedError, match="stack_outputs"):
        mk({"targets": ["binary"], "stack_outputs": False})
    with pytest.raises(NotImplementedError, match="output_dtype 'float16'"):
        mk({"targets": ["binary"], "output_dtype": "float16"})
    with pytest.raises(NotImplementedError, match="33 stacked channels"):
        mk({"targets": [LC._aff(affinity_mode="deepem", offsets=[[0, 0, i] for i in range(33)])]})
    with pytest.raises(NotImplementedError, match="5 distinct erosions"):
        mk({"targets": [{"name": "binary", "kwargs": {"erosion": i}} for i in range(5)]})
    with pytest.raises(NotImplementedError, match="half-size \\(0, 11, 11\\)"):
        mk({"targets": ["binary"], "erosion": 11})
    with pytest.raises(NotImplementedError, match="9 segment_id"):
        mk({"targets": [{"name": "binary", "kwargs": {"segment_id": list(range(1, 10))}}]})
    assert mk({"targets": ["binary"], "erosion": 10}).sources == [((0, 10, 10),)]


def test_labels_stay_integers_on_the_host_side():
    plan = LabelTargetTransform.from_config({"targets": ["binary"]})
    with pytest.raises(TypeError, match="2\\^24"):
        plan(torch.zeros(1, 2, 3, 4))
    with pytest.raises(TypeError, match="2\\^24"):
        labels_to_int32(np.zeros((2, 3, 4), dtype=np.float64))
    with pytest.raises(ValueError, match="outside int32"):
        labels_to_int32(np.array([0, 2 ** 31], dtype=np.int64))
    with pytest.raises(ValueError, match="outside int32"):
        labels_to_int32(torch.tensor([0, 2 ** 32 - 1], dtype=torch.int64))
    big = labels_to_int32(np.array([1 + 2 ** 24, 2 ** 31 - 1, -1], dtype=np.int64))
    assert big.dtype == np.int32 and big.tolist() == [1 + 2 ** 24, 2 ** 31 - 1, -1]
    assert labels_to_int32(np.array([65535], dtype=np.uint16)).tolist() == [65535]
    assert labels_to_int32(torch.tensor([3], dtype=torch.uint8)).dtype == torch.int32
    with pytest.raises(ValueError, match="\\(B, D, H, W\\) or \\(B, 1, D, H, W\\)"):
        plan(torch.zeros(2, 3, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        plan(torch.zeros(1, 2, 3, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        next(device_target_batches(iter([{"image": torch.zeros(1, 1, 2, 3, 4), "label": torch.zeros(1, 2, 3, 4, dtype=torch.int32)}]),
                                   plan, "cpu"))


# ---------------------------------------------------------------------------------------------------------------- the module
class Passthrough(nn.Module):
    """the image IS the logits (times a trainable 1); with `ds` a half-resolution output rides along"""

    def __init__(self, ds=False):
        super().__init__()
        self.scale = nn.Parameter(torch.ones(()))
        self.ds = ds

    def forward(self, x):
        y = x * self.scale
        return {"output": y, "ds_1": F.avg_pool3d(y, 2)} if self.ds else y


def _tensors(seed=0, shape=(2, 3, 4, 6, 8)):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * 3
    t = (torch.rand(shape, generator=g) > 0.6).float()
    lm = torch.rand(shape, generator=g) > 0.35
    bm = (torch.rand((shape[0], 1) + shape[2:], generator=g) > 0.25).float()
    return x, t, lm, bm


BCE = {"function": "WeightedBCEWithLogitsLoss", "weight": 1.0, "kwargs": {"reduction": "mean"}}


def test_label_mask_is_sliced_by_target_slice_and_multiplied_with_the_batch_mask():
    x, t, lm, bm = _tensors()
    terms = [dict(BCE, pred_slice="0:2", target_slice="0:2"), dict(BCE, weight=0.5, pred_slice="2:3", target_slice="2:3")]
    m = ConnectomicsModule(loss_cfg(terms, False), model=Passthrough())

    def want(mask):
        xc = x.clamp(-20, 20)
        a = lm[:, 0:2].float() * (1.0 if mask is None else mask)
        b = lm[:, 2:3].float() * (1.0 if mask is None else mask)
        return weighted_bce_with_logits(xc[:, 0:2], t[:, 0:2] * lm[:, 0:2], a) + 0.5 * weighted_bce_with_logits(xc[:, 2:3], t[:, 2:3] * lm[:, 2:3], b)

    for mask in (None, bm):
        for form in (lm, lm.float()):                        # bool, and the device transform's fp32 0 / 1 form
            total, parts = m._compute_loss(x, t, mask, form)
            assert torch.allclose(total, want(mask), rtol=1e-6), (mask is None, form.dtype)
            assert len(parts) == 3
    # no target_slice: all channels
    m_all = ConnectomicsModule(loss_cfg([BCE], False), model=Passthrough())
    total, _ = m_all._compute_loss(x, t, bm, lm)
    assert torch.allclose(total, weighted_bce_with_logits(x.clamp(-20, 20), t * lm, lm.float() * bm), rtol=1e-6)
    # a term's own mask_slice, the batch mask and the label mask are three factors of one valid mask
    lab4 = torch.cat([t, (torch.rand(2, 1, 4, 6, 8) > 0.3).float()], dim=1)
    lm4 = torch.cat([lm, torch.ones(2, 1, 4, 6, 8, dtype=torch.bool)], dim=1)
    m_own = ConnectomicsModule(loss_cfg([dict(BCE, target_slice="0:3", mask_slice="3:4")], False), model=Passthrough())
    total, _ = m_own._compute_loss(x, lab4, bm, lm4)
    assert torch.allclose(total, weighted_bce_with_logits(x.clamp(-20, 20), t * lm, lab4[:, 3:4] * bm * lm.float()), rtol=1e-6)
    # a loss that sees masks through its inputs (torch's BCE): masked logits read as the clamp minimum, masked targets as 0
    m_plain = ConnectomicsModule(loss_cfg([{"function": "BCEWithLogitsLoss", "weight": 1.0}], False), model=Passthrough())
    total, _ = m_plain._compute_loss(x, t, None, lm)
    assert torch.allclose(total, F.binary_cross_entropy_with_logits(x.clamp(-20, 20).masked_fill(~lm, -20.0), t * lm), rtol=1e-6)


def test_batch_without_label_mask_is_unchanged():
    x, t, lm, bm = _tensors(1)
    terms = [dict(BCE, pred_slice="0:2", target_slice="0:2"), {"function": "DiceLoss", "weight": 1.0, "kwargs": {"sigmoid": True}}]
    m = ConnectomicsModule(loss_cfg(terms, True), model=Passthrough(ds=True))
    batch = {"image": x, "label": t, "mask": bm}
    a = m.training_step(batch)
    b, _ = m._compute_loss(m(x), t, bm)
    c, _ = m._compute_loss(m(x), t, bm, None)
    assert torch.equal(a, b) and torch.equal(a, c)
    # an all-true label mask changes nothing either; a real one does, through training_step, validation_step, fit and validate
    ones = torch.ones_like(lm)
    assert torch.allclose(m.training_step({**batch, "label_mask": ones}), a, rtol=1e-6)
    masked = m.training_step({**batch, "label_mask": lm})
    assert not torch.allclose(masked, a, rtol=1e-3)
    want, _ = m._compute_loss(m(x), t, bm, lm)
    assert torch.equal(masked, want)
    m.eval()
    assert torch.equal(m.validation_step({**batch, "label_mask": lm})["val_loss_total"], want.detach())
    assert validate(m, [{**batch, "label_mask": lm}], device="cpu")["val_loss_total"] == pytest.approx(float(want.detach()), rel=1e-6)
    # fit() hands the key on: the first logged loss is the masked one
    from pytorch_connectomics_amd.config import ConfigNode, schema_defaults
    m_fit = ConnectomicsModule(ConfigNode(schema_defaults()), model=Passthrough())
    one = {"image": x[:, :1], "label": t[:, :1], "label_mask": lm[:, :1]}
    want_fit, _ = m_fit._compute_loss(m_fit(one["image"]), one["label"], None, one["label_mask"])
    plain_fit, _ = m_fit._compute_loss(m_fit(one["image"]), one["label"], None)
    history, _ = fit(m_fit, iter([one]), max_steps=1, device=torch.device("cpu"), log=None)
    assert history[0] == pytest.approx(float(want_fit.detach()), rel=1e-6) and abs(float((plain_fit - want_fit).detach())) > 1e-4


def test_label_mask_dtype_and_shape_errors():
    x, t, lm, _ = _tensors(2)
    m = ConnectomicsModule(loss_cfg([BCE], False), model=Passthrough())
    with pytest.raises(TypeError, match="label_mask must have dtype torch.bool, got torch.uint8"):
        m._compute_loss(x, t, None, lm.to(torch.uint8))
    with pytest.raises(TypeError, match="label_mask must have dtype torch.bool, got torch.float64"):
        check_label_mask(lm.double(), t)
    with pytest.raises(ValueError, match="label_mask must have the same batch, channel, and spatial shape as labels: "
                                         "label_mask=\\(2, 1, 4, 6, 8\\), labels=\\(2, 3, 4, 6, 8\\)"):
        m._compute_loss(x, t, None, lm[:, :1])
    with pytest.raises(ValueError, match="label_mask must have the same batch"):
        m.training_step({"image": x, "label": t, "label_mask": lm[..., :7]})
    assert check_label_mask(lm, t).dtype == torch.float32 and check_label_mask(lm.float(), t).dtype == torch.float32


def test_deep_supervision_resizes_the_label_mask_by_the_invalid_area_rule():
    lm = torch.ones(1, 2, 4, 4, 4)
    lm[0, 0, 0, 0, 0] = 0                                    # one invalid fine voxel: its whole coarse voxel is invalid
    lm[0, 1, 2:, 2:, 2:] = 0
    out = resize_label_mask_to_output(lm, torch.zeros(1, 2, 2, 2, 2))
    want = torch.ones(1, 2, 2, 2, 2)
    want[0, 0, 0, 0, 0] = 0
    want[0, 1, 1, 1, 1] = 0
    assert torch.equal(out, want) and out.dtype == torch.float32
    assert resize_label_mask_to_output(lm, torch.zeros(1, 2, 4, 4, 4)) is lm
    # the reference's own statement of the rule, on a random mask and a non-integer ratio
    g = torch.Generator().manual_seed(5)
    r = torch.rand(2, 3, 6, 9, 8, generator=g) > 0.2
    ref = F.interpolate((~r).float(), size=(3, 4, 4), mode="area") <= 0.0
    assert torch.equal(resize_label_mask_to_output(r.float(), torch.zeros(2, 3, 3, 4, 4)) > 0, ref)
    # through the module: the coarse scale's term sees the resized mask
    x, t, lmask, _ = _tensors(3, (2, 3, 4, 6, 8))
    m = ConnectomicsModule(loss_cfg([BCE], True), model=Passthrough(ds=True))
    outs = m(x)
    total, _ = m._compute_loss(outs, t, None, lmask)
    coarse_t = F.interpolate(t, size=(2, 3, 4), mode="trilinear", align_corners=False).clamp(-1, 1)
    coarse_m = (F.interpolate((~lmask).float(), size=(2, 3, 4), mode="area") <= 0.0).float()
    want = weighted_bce_with_logits(outs["output"].clamp(-20, 20), t * lmask, lmask.float()) \
        + 0.5 * weighted_bce_with_logits(outs["ds_1"].clamp(-20, 20), coarse_t * coarse_m, coarse_m)
    assert torch.allclose(total, want, rtol=1e-6)


def test_per_channel_bce_on_an_affinity_target_matches_the_reference_orchestrator(golden):
    """The reference LossOrchestrator's total and gradient for a PerChannelBCEWithLogitsLoss term on a 3-channel affinity target with
    its label_mask (tests/golden/make_golden_label_targets.py), matched as closely as the fixtures of loss_orchestration.npz are."""
    cfg = loss_cfg([{"function": "PerChannelBCEWithLogitsLoss", "weight": 1.0, "kwargs": {}}], False)
    m = ConnectomicsModule(cfg, model=Passthrough())
    x = torch.from_numpy(golden["orch__logits"]).requires_grad_(True)
    labels = torch.from_numpy(golden["orch__labels"].astype(np.float32))
    lmask = torch.from_numpy(golden["orch__label_mask"])
    assert lmask.dtype == torch.bool and not bool(lmask.all()) and bool(lmask.any())
    total, _ = m._compute_loss(x, labels, None, lmask)
    total.backward()
    assert float(total.detach()) == pytest.approx(float(golden["orch__total"]), rel=3e-6)
    assert torch.allclose(x.grad, torch.from_numpy(golden["orch__grad"]), rtol=2e-5, atol=1e-8)
    without, _ = m._compute_loss(x.detach(), labels, None)
    assert abs(float(without) - float(total.detach())) > 1e-3 * abs(float(total.detach()))          # the mask matters in this fixture

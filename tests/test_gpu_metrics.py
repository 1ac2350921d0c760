"""GPU checks of the evaluation-metric count kernel (csrc/metric_kernels.hip) and of everything built on it.

The counts are integers: every comparison is torch.equal on int64 against the torch reference of tests/metric_cases.py, computed once
per case on the CPU from the same values, and the table always sums to the number of voxels."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import metric_cases as MC  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ["jaccard", "dice", "accuracy"]


def _ops():
    from pytorch_connectomics_amd import hip_ops as ops
    return ops


def _metrics():
    from pytorch_connectomics_amd.training import metrics as M
    return M


def test_tile_size_is_the_one_the_cases_assume():
    from pytorch_connectomics_amd import _native as nat
    tiles = nat.lib().pytc_confusion_tiles
    assert tiles(0) == 0 and tiles(1) == 1 and tiles(MC.TILE) == 1 and tiles(MC.TILE + 1) == 2 and tiles(2 * MC.TILE + 3) == 3
    assert tiles(int(np.prod(MC.VOLUME[2:]))) == 16


@pytest.mark.parametrize("layout", MC.LAYOUTS)
@pytest.mark.parametrize("C", MC.CLASSES)
def test_counts_equal_the_reference_at_every_size(C, layout):
    ops = _ops()
    seen_n, seen_kind = set(), set()
    for ri in range(len(MC.R_SIZES)):
        base, target, mode, pthr, tthr, want, N, R = MC.sized_case(C, layout, ri)
        x = MC.logits_view(base.cuda(), C, layout)
        assert x.shape == (N, C, R)
        got = ops.confusion_counts(x, target.cuda(), target_mode=mode, pred_threshold=pthr, target_threshold=tthr)
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), want), (C, layout, R, N, mode, target.dtype)
        assert int(got.sum()) == N * R and int(got[-1]) == 0
        seen_n.add(N)
        seen_kind.add((mode, target.dtype))
    assert seen_n == {1, 3} and seen_kind == set(MC.target_kinds_for(C))


@pytest.mark.parametrize("layout", MC.LAYOUTS)
def test_multi_tile_volume(layout):
    base, target, want = MC.volume_case(layout)
    N, C = MC.VOLUME[:2]
    x = MC.logits_view(base.cuda(), C, layout)
    assert x.shape == MC.VOLUME
    got = _ops().confusion_counts(x, target.cuda())
    assert torch.equal(got.cpu(), want) and int(got.sum()) == N * int(np.prod(MC.VOLUME[2:]))
    # the label without its channel axis, as float and as uint8, and a one-hot target of the same classes
    for t in (target[:, 0].float(), target.to(torch.uint8)):
        assert torch.equal(_ops().confusion_counts(x, t.cuda()).cpu(), want)
    onehot = torch.nn.functional.one_hot(target[:, 0], C).permute(0, 4, 1, 2, 3).float()
    assert torch.equal(_ops().confusion_counts(x, onehot.cuda(), target_mode="dense").cpu(), want)
    assert torch.equal(_ops().confusion_counts(x, onehot.contiguous().cuda(), target_mode="dense").cpu(), want)


def test_special_values():
    ops = _ops()
    inf, nan = float("inf"), float("nan")
    x = torch.tensor([[inf, nan, inf], [2.0, 2.0, 1.0], [1.0, 1.0, 1.0], [-inf, -inf, -inf], [0.0, -0.0, -1.0], [nan, nan, 5.0]]).t()[None]
    t = torch.tensor([[1.9, -0.5, 0.0, 2.0, 2.999, 1.0]])
    want = torch.zeros(10, dtype=torch.int64)
    for tt, pp in ((1, 1), (0, 0), (0, 0), (2, 0), (2, 0), (1, 0)):          # [inf, nan, inf] -> 1; ties, all-equal, NaN first -> 0
        want[tt * 3 + pp] += 1
    assert torch.equal(MC.reference_counts(x, t, "index"), want)
    for xx in (x.cuda(), x.contiguous().cuda()):
        assert torch.equal(ops.confusion_counts(xx, t.cuda()).cpu(), want)
    assert torch.equal(ops.confusion_counts(x.cuda(), x.cuda().contiguous(), target_mode="dense").cpu(),
                       MC.reference_counts(x, x, "dense"))
    xb = torch.tensor([[[0.5, 0.5000001, nan, -0.0, inf, -inf]]])
    tb = torch.tensor([[1, 1, 1, 0, 0, 0]])
    for dtype in (torch.uint8, torch.int64, torch.float32):
        got = ops.confusion_counts(xb.cuda(), tb.to(dtype).cuda(), pred_threshold=0.5)
        assert got.tolist() == [2, 1, 2, 1, 0]                            # x == threshold and NaN are class 0
    got = ops.confusion_counts(xb.cuda(), tb.float().cuda(), pred_threshold=-0.0)        # -0.0 > -0.0 is false, 0.5 > -0.0 true
    assert got.tolist() == [2, 1, 1, 2, 0]
    got = ops.confusion_counts(xb.cuda(), torch.tensor([[0.5, 0.50001, nan, -1.0, inf, 3.0]]).cuda(), target_mode="threshold",
                               pred_threshold=0.5, target_threshold=0.5)
    assert torch.equal(got.cpu(), MC.reference_counts(xb, torch.tensor([[0.5, 0.50001, nan, -1.0, inf, 3.0]]), "threshold"))


@pytest.mark.parametrize("C", [1, 3, 32])
def test_invalid_labels_are_counted_apart_and_refused_by_compute(C):
    ops, M = _ops(), _metrics()
    K, R = max(C, 2), MC.TILE + 37
    base = MC.logits_base(2, C, (R,), "ncdhw", 5)
    for dtype, bad in ((torch.int64, [-1, K, 1 << 40, -(1 << 40)]), (torch.uint8, [255, K]),
                       (torch.float32, [-1.0, float(K), float("nan"), float("inf"), -float("inf"), 1e30])):
        t = MC.make_target(2, C, (R,), "index", dtype, 3)
        flat = t.reshape(-1)
        for i, v in enumerate(bad):
            flat[17 + 301 * i] = v
            flat[R + 5 + 64 * i] = v
        want = MC.reference_counts(base, t, "index")
        assert int(want[-1]) == 2 * len(bad) and int(want.sum()) == 2 * R
        st = M.ConfusionState(C)
        st.update(base.cuda(), t.cuda())
        assert torch.equal(st.table(), want), (C, dtype)
        with pytest.raises(ValueError, match=f"{2 * len(bad)} voxels"):
            st.compute(NAMES)


@pytest.mark.parametrize("name,x,t,cells", MC.wave_cases(), ids=[c[0] for c in MC.wave_cases()])
def test_one_wave_one_cell_and_one_wave_sixty_four_cells(name, x, t, cells):
    got = _ops().confusion_counts(x.cuda(), t.cuda()).cpu()
    want = torch.zeros_like(got)
    for cell, n in cells.items():
        want[cell] = n
    assert torch.equal(got, want) and torch.equal(MC.reference_counts(x, t, "index"), want)
    # the same 64 voxels as the 64 lanes of one wave: the channels-last form, and a base address no 16-byte vector can start at
    xc = x.permute(0, 2, 1).contiguous().cuda().permute(0, 2, 1)
    assert torch.equal(_ops().confusion_counts(xc, t.cuda()).cpu(), want)
    wide = torch.zeros(1, x.shape[1], 65, device="cuda")
    wide[..., 1:] = x.cuda()
    assert wide[..., 1:].data_ptr() % 16 == 4
    assert torch.equal(_ops().confusion_counts(wide[..., 1:], t.cuda()).cpu(), want)


def test_updates_add_reset_zeroes_and_buffers_are_not_overrun():
    ops, M = _ops(), _metrics()
    from pytorch_connectomics_amd import _native as nat
    base, target, mode, pthr, tthr, want, N, R = MC.sized_case(5, "channels_last", 7)
    x, t = MC.logits_view(base.cuda(), 5, "channels_last"), target.cuda()
    st = M.ConfusionState(5)
    for _ in range(2):
        st.update(x, t, pred_threshold=pthr, target_mode=mode, target_threshold=tthr)
    assert torch.equal(st.table(), 2 * want)
    st.reset()
    assert int(st.table().sum()) == 0
    st.update(x, t, pred_threshold=pthr, target_mode=mode, target_threshold=tthr)
    assert torch.equal(st.table(), want)
    # guarded allocations: the kernels write their partial rows and the table, nothing beside them
    n_part = N * nat.lib().pytc_confusion_tiles(R) * 26
    part = torch.full((n_part + 64,), -7, dtype=torch.int32, device="cuda")
    table = torch.full((26 + 16,), -7, dtype=torch.int64, device="cuda")
    table[8:34] = 0
    ops.confusion_counts(x, t, table[8:34], target_mode=mode, pred_threshold=pthr, target_threshold=tthr, _partial=part[32:32 + n_part])
    assert torch.equal(table[8:34].cpu(), want)
    assert bool((table[:8] == -7).all()) and bool((table[34:] == -7).all())
    assert bool((part[:32] == -7).all()) and bool((part[32 + n_part:] == -7).all()) and int(part[32:32 + n_part].sum()) == N * R


def test_refusals_on_the_device():
    ops = _ops()
    with pytest.raises(NotImplementedError, match="C = 33"):
        ops.confusion_counts(torch.zeros(1, 33, 8, device="cuda"), torch.zeros(1, 8, device="cuda"))
    with pytest.raises(NotImplementedError, match="C = 33"):
        _metrics().ConfusionState(33).update(torch.zeros(1, 33, 8, device="cuda"), torch.zeros(1, 8, device="cuda"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.confusion_counts(torch.zeros(1, 2, 8), torch.zeros(1, 8))
    with pytest.raises(ValueError, match="float32, int64 or uint8"):
        ops.confusion_counts(torch.zeros(1, 2, 8, device="cuda"), torch.zeros(1, 8, device="cuda", dtype=torch.int32))
    with pytest.raises(ValueError, match="threshold target needs"):
        ops.confusion_counts(torch.zeros(1, 2, 8, device="cuda"), torch.zeros(1, 8, device="cuda"), target_mode="threshold")
    # the state casts a label dtype the kernel does not read, once
    st = _metrics().ConfusionState(2)
    st.update(torch.zeros(1, 2, 8, device="cuda"), torch.ones(1, 8, device="cuda", dtype=torch.int32))
    assert st.table().tolist() == [0, 0, 8, 0, 0]
    # the C ABI refuses what the wrapper refuses
    from pytorch_connectomics_amd import _native as nat
    import ctypes as C
    z = torch.zeros(64, device="cuda")
    s3 = (C.c_int64 * 3)(8, 8, 1)
    p = lambda t: C.c_void_p(t.data_ptr())                                                            # noqa: E731
    assert nat.lib().pytc_confusion_counts(p(z), p(z), p(z), p(z), 1, 33, 1, s3, s3, 0, 0, 0.5, 0.5, None) == nat.ERR_UNSUPPORTED
    assert nat.lib().pytc_confusion_counts(p(z), p(z), p(z), p(z), 1, 2, 1, s3, s3, 0, 1, 0.5, 0.5, None) == nat.ERR_INVALID


# ---- module, profiler, CLI -----------------------------------------------------------------------------------------------------
def _module(out_channels, losses):
    from pytorch_connectomics_amd.config import ConfigNode, schema_defaults
    from pytorch_connectomics_amd.training.module import ConnectomicsModule
    c = ConfigNode(schema_defaults())
    c.optimization.precision = "32"
    c.model.arch.type = "monai_basic_unet3d"
    c.model.out_channels = out_channels
    c.model.input_size = [16, 32, 32]
    c.model.monai = {**c.model.monai, "filters": [8, 16], "norm": "group", "num_groups": 1}
    c.model.loss.losses = losses
    c.evaluation.enabled = True
    c.evaluation.metrics = NAMES + ["adapted_rand"]
    torch.manual_seed(11)
    return ConnectomicsModule(c).cuda()


@pytest.mark.parametrize("classes", [1, 3])
def test_validate_counts_what_torch_counts_from_the_same_outputs(classes):
    from pytorch_connectomics_amd.training.module import validate
    losses = None if classes == 1 else [{"function": "CrossEntropyLoss", "weight": 1.0, "target_slice": "0:1"}]
    m = _module(classes, losses)
    g = torch.Generator().manual_seed(classes)
    batches = [{"image": torch.rand((2, 1, 16, 32, 32), generator=g),
                "label": torch.randint(0, max(classes, 2), (2, 1, 16, 32, 32), generator=g).float()} for _ in range(2)]
    m.eval()
    with torch.no_grad():
        outs = [m(b["image"].cuda()) for b in batches]
        for b in batches:
            m.validation_step({k: v.cuda() for k, v in b.items()})
    want = sum(MC.reference_counts(o, b["label"], "index", 0.5) for o, b in zip(outs, batches))
    assert torch.equal(m._val_state.table(), want) and int(want.sum()) == 2 * 2 * 16 * 32 * 32
    m._val_state.reset()
    m.train()
    got = validate(m, batches, device=torch.device("cuda"))
    assert m.training and sorted(got) == ["val_accuracy", "val_dice", "val_jaccard", "val_loss_total"]
    for k, v in _metrics().metrics_from_counts(want, classes, NAMES).items():
        assert got["val_" + k] == v
    assert int(m._val_state.table().sum()) == 0


def test_a_metric_update_launches_no_torch_elementwise_op():
    """One update on CUDA tensors (a channels-last view, a label slice) runs the two HIP launches and no aten:: element-wise,
    reduction, comparison or copy op."""
    M = _metrics()
    base, target, want = MC.volume_case("slice_channels_last")
    x = MC.logits_view(base.cuda(), 3, "slice_channels_last")
    labels = torch.cat([target, target], dim=1).float().cuda()
    st = M.ConfusionState(3)
    st.update(x, labels[:, 1:2])                                          # warm-up: the table, the library
    torch.cuda.synchronize()
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        st.update(x, labels[:, 1:2])
        torch.cuda.synchronize()
    names = {e.key for e in prof.key_averages() if e.key.startswith("aten::")}
    allowed = {"aten::empty", "aten::empty_strided", "aten::detach", "aten::alias", "aten::slice", "aten::select", "aten::unsqueeze",
               "aten::as_strided", "aten::view", "aten::_unsafe_view", "aten::reshape"}
    assert names <= allowed, sorted(names - allowed)
    assert torch.equal(st.table(), 2 * want)


CLI_YAML = """
experiment_name: metrics
save_path: {save}
default:
  optimization: {{precision: "32"}}
  model:
    arch: {{type: mednext_custom}}
    in_channels: 1
    out_channels: 1
    mednext: {{base_channels: 8, exp_r: 2, kernel_size: 3, block_counts: [1,1,1,1,1,1,1,1,1]}}
  inference:
    window: {{window_size: [32, 32, 32], overlap: 0.5, blending: bump, sw_batch_size: 4}}
    model: {{channel_activations: [{{channels: ":", activation: sigmoid}}]}}
  data:
    image_transform: {{normalize: none}}
  evaluation: {{enabled: {enabled}, metrics: [jaccard, dice, accuracy, adapted_rand], prediction_threshold: 0.45}}
test:
  data:
    test: {{image: "{img}", label: "{lab}"}}
"""


def test_cli_test_mode_writes_the_metrics(tmp_path):
    from pytorch_connectomics_amd.inference.artifact import read_prediction_artifact
    from pytorch_connectomics_amd.main import binary_jaccard, main
    rng = np.random.default_rng(0)
    np.save(tmp_path / "img.npy", rng.random((34, 36, 40), dtype=np.float32))
    lab = (rng.random((34, 36, 40)) > 0.5).astype(np.uint16) * 9                   # an instance-style label: > 1, a dtype to cast
    np.save(tmp_path / "lab.npy", lab)
    results = {}
    for enabled in ("false", "true"):
        cfg = tmp_path / f"cfg_{enabled}.yaml"
        cfg.write_text(CLI_YAML.format(save=tmp_path / enabled, img=tmp_path / "img.npy", lab=tmp_path / "lab.npy", enabled=enabled))
        results[enabled] = main(["--config", str(cfg), "--mode", "test"])
        on_disk = json.loads((tmp_path / enabled / "results" / "img_metrics.json").read_text())
        assert {k: on_disk[k] for k in ("jaccard",)} == {k: results[enabled][k] for k in ("jaccard",)}
    pred = torch.from_numpy(read_prediction_artifact(tmp_path / "false" / "results" / "img_prediction.h5"))[0]
    label = torch.from_numpy(lab.astype(np.int64))
    assert "dice" not in results["false"] and results["false"]["jaccard"] == binary_jaccard(pred, label)
    want = _metrics().metrics_from_counts(MC.reference_counts(pred[None, None], label[None, None], "threshold", 0.45, 0.0), 1, NAMES)
    assert {k: results["true"][k] for k in NAMES} == want and "adapted_rand" not in results["true"]


def test_tutorial_minimal_multiclass_eval_validates_while_it_trains(tmp_path):
    """tutorials/minimal_multiclass_eval.yaml as committed (only its output directory moved): two training steps with a validation
    epoch after each, on one-channel class-index labels."""
    from pytorch_connectomics_amd.config import load_config
    from pytorch_connectomics_amd.training.module import ConnectomicsModule, fit
    root = Path(__file__).resolve().parent.parent
    cfg = load_config(root / "tutorials" / "minimal_multiclass_eval.yaml", mode="train", overrides=[f"save_path={tmp_path}"])
    torch.manual_seed(int(cfg.system.seed))
    module = ConnectomicsModule(cfg)
    g = torch.Generator().manual_seed(1)
    patch = tuple(cfg.data.dataloader.patch_size)

    def batch():
        return {"image": torch.rand((2, 1) + patch, generator=g), "label": torch.randint(0, 3, (2, 1) + patch, generator=g).float()}
    val = [batch(), batch()]
    history, _ = fit(module, iter([batch(), batch()]), max_steps=2, device=torch.device("cuda"), log=None, val_batches=val, val_every=1)
    assert len(history) == 2 and [r["step"] for r in module.val_history] == [1, 2]
    for r in module.val_history:
        assert sorted(r) == ["step", "val_accuracy", "val_dice", "val_jaccard", "val_loss_total"]
        assert all(0.0 <= r[k] <= 1.0 for k in ("val_accuracy", "val_dice", "val_jaccard")) and np.isfinite(r["val_loss_total"])
        assert r["val_dice"] >= r["val_jaccard"]

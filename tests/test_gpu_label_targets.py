"""GPU checks of the label-target kernels (csrc/label_target_kernels.hip) and of everything built on them.

Everything here is an integer or a boolean: every comparison is torch.equal / array_equal, against the fixture recorded from the
reference's own functions (tests/golden/label_targets.npz) or, for the tile-shaped cases, the gather-form numpy model of
tests/label_target_cases.py.  No tolerance exists in this file."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import label_target_cases as LC  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "label_targets.npz"


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _ops():
    from pytorch_connectomics_amd import hip_ops as ops
    return ops


def _plan(cfg):
    from pytorch_connectomics_amd.data import LabelTargetTransform
    return LabelTargetTransform.from_config(cfg)


def _guarded(label: np.ndarray, guard: int = 4100):
    """the label inside a larger allocation of another id: a read beyond the sample would meet ids the model never saw"""
    flat = torch.full((label.size + 2 * guard,), 7777, dtype=torch.int32, device="cuda")
    flat[guard:guard + label.size] = torch.from_numpy(label.reshape(-1)).cuda()
    return flat[guard:guard + label.size].view(label.shape)


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_erosion_kernel_equals_the_reference(name, golden):
    label = torch.from_numpy(golden[f"{name}__label"]).cuda()
    for half in LC.CASES[name]["erode"]:
        got = _ops().seg_erode_instance(label, half)
        assert got.dtype == torch.int32 and got.shape == label.shape
        assert torch.equal(got.cpu(), torch.from_numpy(golden[f"{name}__erode_{half[0]}_{half[1]}_{half[2]}"])), (name, half)
    assert torch.equal(label.cpu(), torch.from_numpy(golden[f"{name}__label"]))          # the input is untouched


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_transform_equals_the_reference_in_both_mask_dtypes(name, golden):
    label = torch.from_numpy(golden[f"{name}__label"]).cuda()
    for k, cfg in enumerate(LC.CASES[name]["configs"]):
        plan = _plan(cfg)
        want = torch.from_numpy(golden[f"{name}__{k}__values"].astype(np.float32))
        want_mask = golden.get(f"{name}__{k}__mask")
        assert plan.channels == want.shape[1] and plan.uses_mask == (want_mask is not None)
        for mask_dtype in (torch.bool, torch.float32):
            out = plan(label if mask_dtype == torch.bool else label[:, None], mask_dtype=mask_dtype)
            assert out["label"].dtype == torch.float32 and torch.equal(out["label"].cpu(), want), (name, k)
            if want_mask is None:
                assert "label_mask" not in out
            else:
                m = out["label_mask"]
                assert m.dtype == mask_dtype and torch.equal(m.cpu(), torch.from_numpy(want_mask).to(mask_dtype)), (name, k, mask_dtype)


def test_big_ids_stay_apart():
    """2^24 and 2^24 + 1 touch in the label: as floats they are one id and their edge would read as connected"""
    label = LC.make_label("big_ids")
    assert np.float32(LC.BIG_A) == np.float32(LC.BIG_B)
    out = _plan(LC.CASES["big_ids"]["configs"][0])(torch.from_numpy(label).cuda())
    x_aff = out["label"][0, 2].cpu().numpy()                 # offset (0, 0, 1), deepem: the edge is stored at its destination
    a, b = label[0, :, :, :-1], label[0, :, :, 1:]
    touching = (a == LC.BIG_A) & (b == LC.BIG_B)
    assert touching.any() and not x_aff[:, :, 1:][touching].any()


TILE_CFG = {"targets": [LC._aff(offsets=[[0, 0, 1], [0, 0, -3], [0, 1, 0], [1, 0, 2], [0, 0, 0]], affinity_mode="deepem"),
                        {"name": "instance_boundary", "kwargs": {"edge_mode": "all"}}, "binary",
                        {"name": "polarity", "kwargs": {"exclusive": True}}]}


def _tile_label(shape, seed):
    rng = np.random.default_rng(seed)
    B, D, H, W = shape
    runs = rng.integers(-1, 5, size=(B, D, H, -(-W // 3)))
    return np.repeat(runs, 3, axis=3)[..., :W].astype(np.int32)


def test_tile_shaped_cases_equal_the_model():
    from pytorch_connectomics_amd import _native as nat
    tile = nat.lib().pytc_label_targets_tile()
    assert tile >= 256 and tile % 4 == 0
    w2 = tile // 6 + 3                                       # 2 x 3 x w2 voxels: more than one tile, not a whole number of them;
    w2 += (2 - w2) % 4                                       # w2 = 2 mod 4: rows are not vector-aligned, the sample is
    shapes = [(1, 1, 1, tile + 5), (2, 2, 3, w2)]
    assert shapes[1][3] % 4 != 0 and (2 * 3 * w2) % tile != 0 and 2 * 3 * w2 > tile and (2 * 3 * w2) % 4 == 0
    plan = _plan(TILE_CFG)
    for i, shape in enumerate(shapes):
        label = _tile_label(shape, 9300 + i)
        want, want_mask = LC.model_batch(label, TILE_CFG)
        for mask_dtype, guard in ((torch.bool, 4100), (torch.float32, 4100), (torch.bool, 4099)):     # 4099: a label off 16 bytes
            out = plan(_guarded(label, guard), mask_dtype=mask_dtype)
            assert torch.equal(out["label"].cpu(), torch.from_numpy(want)), shape
            assert torch.equal(out["label_mask"].cpu(), torch.from_numpy(want_mask).to(mask_dtype)), (shape, mask_dtype)
        for half in ((0, 1, 1), (1, 0, 2)):
            got = _ops().seg_erode_instance(_guarded(label).contiguous(), half)
            assert np.array_equal(got.cpu().numpy(), np.stack([LC.model_erode(s, half) for s in label])), (shape, half)


def test_samples_are_isolated(golden):
    """sample 1 is unchanged when sample 0's ids change: no window and no offset crosses a sample"""
    name = "aff12_erosion1"
    label = golden[f"{name}__label"].copy()
    plan = _plan(LC.CASES[name]["configs"][0])
    first = plan(torch.from_numpy(label).cuda())
    label[0] = np.where(label[0] > 0, label[0] + 11, label[0])[:, ::-1].copy()
    second = plan(torch.from_numpy(label).cuda())
    for key in ("label", "label_mask"):
        assert torch.equal(first[key][1], second[key][1]), key
    assert not torch.equal(first["label"][0], second["label"][0])
    er = [_ops().seg_erode_instance(torch.from_numpy(v).cuda(), (1, 1, 1)) for v in (golden[f"{name}__label"], label)]
    assert torch.equal(er[0][1], er[1][1])


def test_refusals():
    from pytorch_connectomics_amd import _native as nat
    ops, lib = _ops(), nat.lib()
    seg = torch.zeros((1, 2, 8, 8), dtype=torch.int32, device="cuda")
    out = torch.empty_like(seg)
    st = ops._stream()
    p = lambda t: C.c_void_p(t.data_ptr())                   # noqa: E731
    INVALID, UNSUPPORTED = nat.ERR_INVALID, nat.ERR_UNSUPPORTED
    # aliasing `out` (the same buffer, and one overlapping it), a null pointer, a half-size of 11
    assert lib.pytc_seg_erode_instance(p(seg), p(seg), 1, 2, 8, 8, 0, 1, 1, st) == INVALID and b"alias" in lib.pytc_last_error()
    both = torch.zeros((2 * seg.numel() - 4,), dtype=torch.int32, device="cuda")
    assert lib.pytc_seg_erode_instance(p(both), C.c_void_p(both.data_ptr() + 4 * (seg.numel() - 4)), 1, 2, 8, 8, 0, 1, 1, st) == INVALID
    assert lib.pytc_seg_erode_instance(None, p(out), 1, 2, 8, 8, 0, 1, 1, st) == INVALID
    assert lib.pytc_seg_erode_instance(p(seg), None, 1, 2, 8, 8, 0, 1, 1, st) == INVALID
    assert lib.pytc_seg_erode_instance(p(seg), p(out), 1, 2, 8, 8, 0, 11, 1, st) == UNSUPPORTED and b"11" in lib.pytc_last_error()
    assert lib.pytc_seg_erode_instance(p(seg), p(out), 1, 2, 8, 8, 10, 10, 10, st) == nat.OK
    with pytest.raises(RuntimeError, match="alias"):
        ops.seg_erode_instance(seg, (0, 1, 1), out=seg)
    # 33 channels, 5 sources, a null pointer
    rows = (nat.LabelChannel * 33)()
    for r in rows:
        r.kind = nat.LABEL_BINARY
    srcs = (C.c_void_p * 5)(*[seg.data_ptr()] * 5)
    vals = torch.empty((1, 33, 2, 8, 8), dtype=torch.float32, device="cuda")
    args = (1, 2, 8, 8, st)
    assert lib.pytc_label_targets(srcs, 1, rows, 33, p(vals), None, 0, *args) == UNSUPPORTED
    assert lib.pytc_label_targets(srcs, 5, rows, 32, p(vals), None, 0, *args) == UNSUPPORTED
    assert lib.pytc_label_targets(srcs, 1, rows, 32, None, None, 0, *args) == INVALID
    assert lib.pytc_label_targets(None, 1, rows, 32, p(vals), None, 0, *args) == INVALID
    assert lib.pytc_label_targets(srcs, 1, None, 32, p(vals), None, 0, *args) == INVALID
    assert lib.pytc_label_targets(srcs, 1, rows, 32, p(seg), None, 0, *args) == INVALID      # values alias the source
    assert lib.pytc_label_targets(srcs, 1, rows, 32, p(vals), None, 0, *args) == nat.OK
    torch.cuda.synchronize()
    assert torch.equal(vals[:, :32].cpu(), torch.zeros(1, 32, 2, 8, 8))
    # the wrappers: CPU tensors, float labels
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.seg_erode_instance(seg.cpu(), (0, 1, 1))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.label_targets([seg.cpu()], rows)
    plan = _plan({"targets": ["binary"]})
    with pytest.raises(RuntimeError, match="no CPU path"):
        plan(seg.cpu())
    with pytest.raises(TypeError, match="2\\^24"):
        plan(seg.float())
    wide = torch.full((1, 2, 8, 8), 2 ** 31, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="outside int32"):
        plan(wide)
    assert torch.equal(plan((wide - 1))["label"].cpu(), torch.ones(1, 1, 2, 8, 8))


def test_tutorial_minimal_affinity_trains_on_an_id_volume(tmp_path):
    """tutorials/minimal_affinity.yaml as committed, on seeded volumes of its own (output directory, volume paths and a smaller patch
    are the only edits): the first batch the loop builds equals the numpy model's batch for the same seed, two steps train, the
    loss stays finite."""
    from pytorch_connectomics_amd.config import load_config
    from pytorch_connectomics_amd.main import main, train_batches
    from pytorch_connectomics_amd.training import ConnectomicsModule
    image, lab = LC.demo_volume(seed=9401, shape=(24, 40, 40), block=(6, 10, 10))
    assert (lab > 2 ** 24).any() and (lab == -1).any()
    np.save(tmp_path / "img.npy", image)
    np.save(tmp_path / "lab.npy", lab.astype(np.int64))                               # a dtype to range-check and convert
    text = (Path(__file__).resolve().parent.parent / "tutorials" / "minimal_affinity.yaml").read_text()
    for old, new in (("outputs/minimal_affinity", str(tmp_path / "out")), ("tests/golden/minimal_affinity_image.npz", str(tmp_path / "img.npy")),
                     ("tests/golden/minimal_affinity_label.npz", str(tmp_path / "lab.npy")), ("[32, 32, 32]", "[16, 32, 32]")):
        assert old in text
        text = text.replace(old, new)
    path = tmp_path / "minimal_affinity.yaml"
    path.write_text(text)
    cfg = load_config(str(path), mode="train")
    torch.manual_seed(int(cfg.system.seed))
    module = ConnectomicsModule(cfg)
    batch = next(iter(train_batches(cfg, module, torch.device("cuda", 0))))
    # the sampler's draws, restated: one offset per axis and sample from the seeded generator
    g = torch.Generator().manual_seed(int(cfg.system.seed))
    patch, ids, imgs = (16, 32, 32), [], []
    for _ in range(2):
        o = [int(torch.randint(0, lab.shape[a] - patch[a] + 1, (1,), generator=g)) for a in range(3)]
        sl = tuple(slice(o[a], o[a] + patch[a]) for a in range(3))
        ids.append(lab[sl])
        imgs.append(image[sl])
    ids = np.stack(ids)
    model_cfg = {"erosion": 1, "targets": [LC._aff(offsets=LC.AFF12, affinity_mode="deepem")]}
    want, want_mask = LC.model_batch(ids, model_cfg)
    assert batch["label"].shape == (2, 12, 16, 32, 32) and torch.equal(batch["label"].cpu(), torch.from_numpy(want))
    assert batch["label_mask"].dtype == torch.float32 and torch.equal(batch["label_mask"].cpu(), torch.from_numpy(want_mask).float())
    assert 0.02 < float(batch["label"].mean()) < 0.98 and 0.02 < float(batch["label_mask"].mean()) < 0.98
    lo, hi = float(image.min()), float(image.max())
    assert torch.allclose(batch["image"][:, 0].cpu(), (torch.from_numpy(np.stack(imgs)).float() - lo) / (hi - lo), atol=1e-6)
    out = main(["--config", str(path), "--mode", "train"])
    assert out["steps"] == 2 and np.isfinite(out["first_loss"]) and np.isfinite(out["last_loss"])
    # stacked channels that do not match the model fail before the first step, naming both numbers
    bad = tmp_path / "bad.yaml"
    bad.write_text(text.replace("out_channels: 12", "out_channels: 3"))
    with pytest.raises(ValueError, match="stack 12 channels.*model.out_channels is 3"):
        main(["--config", str(bad), "--mode", "train"])


def test_fused_bce_dice_path_takes_the_label_mask_as_the_generic_path_does():
    """Fusable terms (weighted BCE + sigmoid Dice on channel slices) with a `label_mask`: the fused kernel reads batch mask x the
    term's label-mask channels as its per-channel weight and gives the generic path's value and gradient (same tolerances as the
    fused-against-generic comparison of tests/test_gpu_training.py: two fp32 reductions of the same terms in another order).  A
    plain BCE that sees masks through its inputs stays off the fused kernel, with a label mask as with a batch mask."""
    from loss_cases import loss_cfg
    from pytorch_connectomics_amd.training.module import ConnectomicsModule
    dev = torch.device("cuda")
    terms = [{"function": "WeightedBCEWithLogitsLoss", "weight": 1.0, "pos_weight": 2.0, "pred_slice": "0:2", "target_slice": "0:2"},
             {"function": "DiceLoss", "weight": 0.5, "kwargs": {"sigmoid": True}, "pred_slice": "0:2", "target_slice": "0:2"},
             {"function": "DiceLoss", "weight": 2.0, "kwargs": {"sigmoid": True}, "pred_slice": "2:3", "target_slice": "2:3"}]
    cfg = loss_cfg(terms, False)
    cfg.model.loss.fused = True
    m = ConnectomicsModule(cfg, model=torch.nn.Identity())
    g = torch.Generator().manual_seed(9500)
    pred0 = (torch.randn(2, 3, 8, 12, 20, generator=g) * 3).to(dev)
    tgt = (torch.rand(2, 3, 8, 12, 20, generator=g) > 0.6).float().to(dev)
    lmask = (torch.rand(2, 3, 8, 12, 20, generator=g) > 0.3).to(dev)
    bmask = (torch.rand(2, 1, 8, 12, 20, generator=g) > 0.2).float().to(dev)
    for mask in (None, bmask):
        for form in (lmask, lmask.float()):
            res = {}
            for fused in (True, False):
                m.fused_loss = fused
                pred = pred0.clone().requires_grad_(True)
                tot, _ = m._compute_loss(pred, tgt, mask, form)
                tot.backward()
                res[fused] = (float(tot.detach()), pred.grad.clone())
            assert res[True][0] == pytest.approx(res[False][0], rel=2e-6)
            assert torch.allclose(res[True][1], res[False][1], rtol=1e-4, atol=1e-9)
    m.fused_loss = True
    plain, _ = m._compute_loss(pred0, tgt, None, None)
    masked, _ = m._compute_loss(pred0, tgt, None, lmask)
    assert abs(float(plain) - float(masked)) > 1e-3
    assert m._fusable(pred0, lmask.float(), list(enumerate(m.loss_terms)))
    m_plain = ConnectomicsModule(loss_cfg([{"function": "BCEWithLogitsLoss", "weight": 1.0}], False), model=torch.nn.Identity())
    m_plain.fused_loss = True
    assert m_plain._fusable(pred0, None, list(enumerate(m_plain.loss_terms)))
    assert not m_plain._fusable(pred0, lmask.float(), list(enumerate(m_plain.loss_terms)))

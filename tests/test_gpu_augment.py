"""GPU checks of the augmentation kernels (csrc/augment_kernels.hip) and of everything built on them.

Every comparison is exact: against the fixture recorded from the reference's own code (tests/golden/augment.npz) or the gather-form
numpy model of tests/augment_cases.py (itself checked against that fixture on the CPU); fp32 results are compared as int32 bits.
No tolerance exists in this file."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import augment_cases as X  # noqa: E402
import label_target_cases as LC  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "augment.npz"


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _mods():
    from pytorch_connectomics_amd import _native as nat
    from pytorch_connectomics_amd import hip_ops as ops
    from pytorch_connectomics_amd.data import augment as A
    return nat, ops, A


def _guarded(arr: np.ndarray, guard: int = 4100):
    """the array inside a larger allocation of a sentinel: a read beyond it would meet values the model never saw"""
    t = torch.from_numpy(np.ascontiguousarray(arr))
    flat = torch.full((arr.size + 2 * guard,), 7777, dtype=t.dtype, device="cuda")
    flat[guard:guard + arr.size] = t.reshape(-1).cuda()
    return flat[guard:guard + arr.size].view(arr.shape)


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.int32)


def _permute(x: np.ndarray, perms):
    """x (N, C, D, H, W) through the gather kernel, one signed permutation per sample"""
    _, ops, _ = _mods()
    host = np.ascontiguousarray(np.array(perms, dtype=np.int32).reshape(x.shape[0], 3))
    out = ops.augment_permute(_guarded(x), torch.from_numpy(host.reshape(-1)).cuda(), host)
    return out.cpu().numpy()


def _tables(rows_per_sample):
    nat = _mods()[0]
    offsets = np.zeros(len(rows_per_sample) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(r) for r in rows_per_sample])
    flat = [r for rows in rows_per_sample for r in rows]
    return np.array(flat, dtype=np.int64).astype(np.int32).reshape(len(flat), nat.AUG_ROW), offsets


def _defects(x: np.ndarray, rows_per_sample):
    """x fp32 (N, C, D, H, W) through the defect kernel, one row list per sample"""
    _, ops, _ = _mods()
    rows, offsets = _tables(rows_per_sample)
    out = ops.augment_defects(_guarded(x), torch.from_numpy(rows.reshape(-1)).cuda() if len(rows) else None,
                              torch.from_numpy(offsets).cuda(), rows, offsets, out=torch.full(x.shape, -3.0, device="cuda"))
    return out.cpu().numpy()


@pytest.mark.parametrize("side", [12, 13])
@pytest.mark.parametrize("channels", [1, 2])
def test_all_48_permutations_of_a_cube(side, channels):
    """ids (one above 2^24, negative ones) and fp32 bit patterns; three samples per launch with different permutations, the middle
    one the identity; 12^3 moves 16-byte vectors, 13^3 single elements"""
    shape = (3, channels, side, side, side)
    ids, img = X.make_ids(shape, side), X.make_image(shape, side + 1)
    assert (ids > 2 ** 24).any() and (ids < 0).any()
    for k in range(0, 48, 2):
        perms = [X.ALL_PERMS[k], (0, 1, 2), X.ALL_PERMS[k + 1]]
        for x in (ids, img):
            got = _permute(x, perms)
            want = np.stack([X.permute_model(x[n], perms[n]) for n in range(3)])
            assert got.dtype == x.dtype and np.array_equal(_bits(got), _bits(want)), (side, channels, perms, x.dtype)


@pytest.mark.parametrize("shape, perms", [
    ((5, 9, 14), X.FLIP_PERMS),                              # non-cubic, W no multiple of 4: flips only
    ((5, 6, 8), X.FLIP_PERMS),                               # ... and the vector path
    ((9, 9, 14), [(1, 0, 2), (-2, 0, -3), (1, -1, 2)]),      # z <-> y: x stays, whole lines
    ((5, 12, 12), [(0, 2, 1), (-1, -3, 1), (0, 2, -2)]),     # y <-> x: tiles, one plane per z
    ((12, 5, 12), [(2, 1, 0), (-3, -2, 0), (2, 1, -1)]),     # z <-> x: tiles, one plane per y
    ((3, 37, 37), X.FLIP_PERMS + [(0, 2, 1), (0, -3, -2)]),  # pytc_augment_tile() + 11 voxels: a ragged tail, single elements
    ((1, 41, 100), X.FLIP_PERMS),                            # pytc_augment_tile() + 4 voxels, vectors
    ((70, 70, 70), [(2, 1, 0), (1, -3, 0), (0, 1, 2), (-2, -3, -1)]),   # more than one 64 x 64 tile per plane, ragged tiles
])
def test_permutations_on_the_shapes_where_the_kernels_can_go_wrong(shape, perms):
    nat = _mods()[0]
    tile = nat.lib().pytc_augment_tile()
    if shape in ((3, 37, 37), (1, 41, 100)):
        assert tile < int(np.prod(shape)) < tile + 12
    x = X.make_ids((len(perms), 2) + shape, 31)
    got = _permute(x, perms)
    want = np.stack([X.permute_model(x[n], perms[n]) for n in range(len(perms))])
    assert np.array_equal(got, want)


def test_identity_batches_launch_nothing():
    _, ops, _ = _mods()
    x = torch.zeros((2, 1, 4, 4, 4), dtype=torch.int32, device="cuda")
    host = np.array([[0, 1, 2], [0, 1, 2]], dtype=np.int32)
    assert ops.augment_permute(x, torch.from_numpy(host.reshape(-1)).cuda(), host) is x
    img = torch.zeros((2, 1, 4, 4, 4), device="cuda")
    off = np.zeros(3, dtype=np.int32)
    assert ops.augment_defects(img, None, torch.from_numpy(off).cuda(), None, off) is img


@pytest.mark.parametrize("name", sorted(X.PURE_CASES))
def test_kernels_equal_the_reference_functions(golden, name):
    """every pure-function case of the fixture (shifts of +-(dim - 1) and +-dim with and without wrap along each axis, translations
    split at 1 and D - 2, fills, lost sections next to each other, interpolation, all rotations) through the kernels"""
    case = X.PURE_CASES[name]
    vol = (X.make_ids if case["ids"] else X.make_image)(case["shape"], case["seed"])
    if case["perm"] is not None:
        got = _permute(vol[None], [case["perm"]])[0]
    else:
        got = _defects(vol[None], [case["rows"]])[0]
    assert np.array_equal(_bits(got), _bits(golden[f"fn__{name}__out"]))


@pytest.mark.parametrize("cls_name", sorted(X.CLASS_CASES))
def test_plan_tables_through_the_kernels_equal_the_reference_classes(golden, cls_name):
    """each reference class, every case, two seeds: the plan's tables applied by `apply_tables` (one upload, both kernels)"""
    _, _, A = _mods()
    for i, case in enumerate(X.CLASS_CASES[cls_name]):
        for seed in case["seeds"][:2]:
            image, label = X.class_case_arrays(cls_name, i, seed)
            perms, rows, offsets = X.class_plan(cls_name, i, seed).draw_batch(1, image.shape[1:])
            batch = {"image": torch.from_numpy(image[None]).cuda()}
            if label is not None:
                batch["label"] = torch.from_numpy(label[None]).cuda()
            out = A.apply_tables(batch, perms, rows, offsets)
            torch.cuda.synchronize()
            assert np.array_equal(_bits(out["image"][0]), _bits(golden[f"cls__{cls_name}__{i}__{seed}__out"])), (cls_name, i, seed)
            if label is not None:
                assert np.array_equal(out["label"][0].cpu().numpy(), golden[f"cls__{cls_name}__{i}__{seed}__label_out"])


@pytest.mark.parametrize("shape", [(2, 6, 9, 11), (1, 6, 8, 12), (1, 3, 37, 37)])
def test_defect_chains_equal_the_model(shape):
    """fills touching every face, a multiply-add before and after a fill, section copies at z = 1 and z = D - 2, and samples with 0, 1
    and 12 rows of every kind in one batch; (2, 6, 9, 11) stores single elements, (1, 6, 8, 12) vectors, (1, 3, 37, 37) a ragged tail"""
    nat, _, A = _mods()
    C_, D, H, W = shape
    dims = (D, H, W)
    faces = [A.fill_row(b, 0.1 * (k + 1), dims) for k, b in enumerate(
        ([0, 1, 0, H, 0, W], [D - 1, D, 0, H, 0, W], [0, D, 0, 2, 0, W], [0, D, H - 1, H, 0, W], [0, D, 0, H, 0, 1], [0, D, 0, H, W - 3, W]))]
    scaled = [A.muladd_row(1.07, 0.03), A.fill_row([1, D, 2, 5, 3, 9], 0.5, dims), A.muladd_row(0.93, -0.02),
              A.fill_row([0, 2, 0, 4, 0, 4], 0.25, dims)]
    copies = [A.copy_row(1, -1, 1), A.copy_row(D - 2, 1, 1)] if D > 3 else [A.copy_row(1, 1, 1)]
    means = [A.copy_row(1, 0, 1)] + ([A.copy_row(2, 0, 1), A.copy_row(D - 2, 0, 1)] if D > 4 else [])
    chain = X.chain_rows(dims, 5)
    assert len(chain) == 12 and {r[0] for r in chain} == {nat.AUG_FILL, nat.AUG_MOVE, nat.AUG_COPY_SECTION, nat.AUG_MULADD}
    per_sample = [[], faces[:1], chain, faces, scaled, copies, means, X.chain_rows(dims, 6)]
    x = X.make_image((len(per_sample),) + shape, 77)
    got = _defects(x, per_sample)
    for n, rows in enumerate(per_sample):
        want = X.defects_model(x[n], rows)
        assert np.array_equal(_bits(got[n]), _bits(want)), (shape, n)
    assert np.array_equal(_bits(got[0]), _bits(x[0]))                             # no rows: a copy, bit for bit
    mul, add = np.float32(1.07), np.float32(0.03)
    m2, a2 = np.float32(0.93), np.float32(-0.02)
    first = (x[4] * mul + add) * m2 + a2                      # numpy's float32 arithmetic: every product and sum rounded
    assert np.array_equal(_bits(got[4][:, 2:, 5:, :]), _bits(first[:, 2:, 5:, :]))
    assert (got[4][:, 1:, 2:5, 4:9] == np.float32(0.5) * m2 + a2).all() and (got[4][:, :2, :4, :4] == np.float32(0.25)).all()


def test_argument_checks_return_their_code_without_launching():
    nat, ops, A = _mods()
    lib, st = nat.lib(), ops._stream()
    INVALID, UNSUPPORTED = nat.ERR_INVALID, nat.ERR_UNSUPPORTED
    p = lambda t: C.c_void_p(t.data_ptr())                   # noqa: E731
    h = lambda a: C.c_void_p(a.ctypes.data)                  # noqa: E731
    x = torch.arange(2 * 4 * 6 * 6, dtype=torch.int32, device="cuda").view(2, 1, 4, 6, 6)
    out = torch.full_like(x, -5)
    ident = np.array([[0, 1, 2], [0, 1, 2]], dtype=np.int32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()     # noqa: E731
    shape = (2, 1, 4, 6, 6)
    perm = lib.pytc_augment_permute
    ident_d = dev(ident)
    assert perm(None, p(out), p(ident_d), h(ident), *shape, st) == INVALID
    assert perm(p(x), None, p(ident_d), h(ident), *shape, st) == INVALID
    assert perm(p(x), p(out), None, h(ident), *shape, st) == INVALID
    assert perm(p(x), p(out), p(ident_d), None, *shape, st) == INVALID
    assert perm(p(x), p(x), p(ident_d), h(ident), *shape, st) == INVALID and b"alias" in lib.pytc_last_error()
    assert perm(p(x), p(out), p(ident_d), h(ident), 2, 1, 4, 0, 6, st) == INVALID
    for bad, code, word in (([[0, 1, 2], [0, 0, 2]], INVALID, b"not a signed permutation"), ([[0, 1, 3], [0, 1, 2]], INVALID, b"names no axis"),
                            ([[0, 1, 2], [-4, 1, 2]], INVALID, b"names no axis"), ([[1, 0, 2], [0, 1, 2]], UNSUPPORTED, b"another length")):
        bad = np.array(bad, dtype=np.int32)
        bad_d = dev(bad)
        assert perm(p(x), p(out), p(bad_d), h(bad), *shape, st) == code and word in lib.pytc_last_error(), bad
    torch.cuda.synchronize()
    assert (out == -5).all()                                 # nothing above launched
    swap = np.array([[0, 2, 1], [0, -3, 1]], dtype=np.int32)                     # y <-> x of a (4, 6, 6) patch keeps the shape
    swap_d = dev(swap)
    assert perm(p(x), p(out), p(swap_d), h(swap), *shape, st) == nat.OK
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.stack([X.permute_model(x.cpu().numpy()[n], swap[n]) for n in range(2)]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.augment_permute(x.cpu(), dev(ident), ident)
    with pytest.raises(ValueError, match="int32"):
        ops.augment_permute(x.double(), dev(ident), ident)
    with pytest.raises(ValueError, match="perm_host"):
        ops.augment_permute(x, dev(ident), ident.astype(np.int64))
    # the defect launch
    img = torch.rand(shape, device="cuda")
    res = torch.full_like(img, -5.0)
    dims = (4, 6, 6)
    good = np.array([A.muladd_row(2.0, 0.0)], dtype=np.int64).astype(np.int32)
    off = np.array([0, 1, 1], dtype=np.int32)
    run = lib.pytc_augment_defects

    def call(rows, offsets, image=img, result=res, rows_dev=True, off_dev=True, n=2):
        rows, offsets = np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(offsets, dtype=np.int32)
        rows_d, offsets_d = dev(rows), dev(offsets)           # both alive over the call: a freed table's memory is the next one's
        return run(p(image) if image is not None else None, p(result) if result is not None else None, p(rows_d) if rows_dev else None,
                   p(offsets_d) if off_dev else None, h(rows), h(offsets), n, 1, *dims, st)
    assert call(good, off, image=None) == INVALID and call(good, off, result=None) == INVALID
    assert call(good, off, rows_dev=False) == INVALID and call(good, off, off_dev=False) == INVALID
    assert call(good, off, result=img) == INVALID and b"alias" in lib.pytc_last_error()
    assert call(good, [1, 1, 1]) == INVALID and call(good, [0, 1, 0]) == INVALID
    rows = lambda *r: np.array(r, dtype=np.int64).astype(np.int32)               # noqa: E731
    for bad, code, word in (
            (rows((7, 0, 0, 0, 0, 0, 0, 0, 0, 0)), INVALID, b"unknown op kind 7"),
            (rows((nat.AUG_FILL, 0, 0, 5, 0, 6, 0, 6, 0, 0)), INVALID, b"fill box"),
            (rows((nat.AUG_MOVE, 0, 3, 0, 1, 0, 0, 0, 0, 0)), INVALID, b"axis 3"),
            (rows((nat.AUG_MOVE, 0, 1, 0, 7, 0, 0, 0, 0, 0)), INVALID, b"slab"),
            (rows((nat.AUG_MOVE, 0, 1, 0, 1, 2 ** 30, 0, 0, 0, 0)), INVALID, b"shift"),
            (rows(A.copy_row(0, 1, 1)), INVALID, b"section 0"), (rows(A.copy_row(3, -1, 1)), INVALID, b"section 3"),
            (rows(A.copy_row(1, 2, 1)), INVALID, b"section 1")):
        assert call(bad, off) == code and word in lib.pytc_last_error(), bad
    two_means = rows(A.copy_row(1, 0, 1), A.copy_row(2, 0, 2))
    assert call(two_means, [0, 2, 2]) == UNSUPPORTED and b"one level of means" in lib.pytc_last_error()
    many = np.repeat(good, nat.AUG_MAX_OPS + 1, axis=0)
    assert call(many, [0, nat.AUG_MAX_OPS + 1, nat.AUG_MAX_OPS + 1]) == UNSUPPORTED and b"at most" in lib.pytc_last_error()
    torch.cuda.synchronize()
    assert (res == -5.0).all()                               # nothing above launched
    assert call(np.repeat(good, nat.AUG_MAX_OPS, axis=0)[:3], [0, 3, 3]) == nat.OK
    torch.cuda.synchronize()
    assert torch.equal(res[0], img[0] * 8.0) and torch.equal(res[1], img[1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.augment_defects(img.cpu(), dev(good), dev(off), good, off)
    with pytest.raises(ValueError, match="float32"):
        ops.augment_defects(x, dev(good), dev(off), good, off)
    with pytest.raises(ValueError, match="signed permutation"):
        A.apply_tables({"image": img}, np.array([[0, 0, 2], [0, 1, 2]]), good[:0], np.zeros(3, dtype=np.int32))
    with pytest.raises(ValueError, match="unknown op kind"):
        A.apply_tables({"image": img}, ident, rows((7, 0, 0, 0, 0, 0, 0, 0, 0, 0)), off)
    with pytest.raises(TypeError, match="int32 or float32"):
        A.apply_tables({"image": img, "label": x.long()}, swap, good[:0], np.zeros(3, dtype=np.int32))


def _tutorial(tmp_path, name, edits=()):
    image, lab = LC.demo_volume(seed=9402, shape=(30, 40, 40), block=(6, 10, 10))
    if not (tmp_path / "img.npy").exists():
        np.save(tmp_path / "img.npy", image)
        np.save(tmp_path / "lab.npy", lab.astype(np.int64))
    text = (ROOT / "tutorials" / f"{name}.yaml").read_text()
    for old, new in ((f"outputs/{name}", str(tmp_path / f"out_{name}")), ("tests/golden/minimal_affinity_image.npz", str(tmp_path / "img.npy")),
                     ("tests/golden/minimal_affinity_label.npz", str(tmp_path / "lab.npy")), ("[32, 32, 32]", "[16, 16, 16]")) + tuple(edits):
        assert old in text, old
        text = text.replace(old, new)
    path = tmp_path / f"{name}_{len(edits)}.yaml"
    path.write_text(text)
    return path, lab


def test_tutorial_minimal_augmented_end_to_end(tmp_path):
    """tutorials/minimal_augmented.yaml with seeded volumes of its own and a 16^3 patch (output directory, volume paths and the patch
    size are the only edits; the file as committed runs in the test below), two batches: the image equals the model applied to the
    unaugmented iterator's image, label and label_mask equal the target model on the permuted id patches; with every block disabled the batches are the unaugmented iterator's, bit for bit; two steps train"""
    from pytorch_connectomics_amd.config import load_config
    from pytorch_connectomics_amd.data import AugmentationPlan
    from pytorch_connectomics_amd.main import main, train_batches
    from pytorch_connectomics_amd.training import ConnectomicsModule
    dev = torch.device("cuda", 0)
    path, lab = _tutorial(tmp_path, "minimal_augmented")
    plain_path, _ = _tutorial(tmp_path, "minimal_affinity")
    off_path, _ = _tutorial(tmp_path, "minimal_augmented", edits=(("enabled: true", "enabled: false"),))
    cfg, plain_cfg, off_cfg = (load_config(str(q), mode="train") for q in (path, plain_path, off_path))
    assert all(not b["enabled"] for b in off_cfg.data.augmentation.values()) and len(off_cfg.data.augmentation) == 6
    torch.manual_seed(int(cfg.system.seed))
    module = ConnectomicsModule(cfg)
    its = [iter(train_batches(c, module, dev)) for c in (cfg, plain_cfg, off_cfg)]
    twin = AugmentationPlan.from_config(cfg.data.augmentation, seed=int(cfg.system.seed))
    assert list(twin.blocks) == ["rotate90_all", "flip", "intensity", "lost_section", "misalignment", "missing_section"]
    g = torch.Generator().manual_seed(int(cfg.system.seed))
    patch = (16, 16, 16)
    model_cfg = {"erosion": 1, "targets": [LC._aff(offsets=LC.AFF12, affinity_mode="deepem")]}
    seen_perm = seen_rows = 0
    for _ in range(2):
        got, plain, off = (next(it) for it in its)
        for key in ("image", "label", "label_mask"):
            assert np.array_equal(_bits(off[key]), _bits(plain[key])), key
        ids = []
        for _ in range(2):                                   # the sampler's draws, restated
            o = [int(torch.randint(0, lab.shape[a] - patch[a] + 1, (1,), generator=g)) for a in range(3)]
            ids.append(lab[tuple(slice(o[a], o[a] + patch[a]) for a in range(3))])
        perms, rows, offsets = twin.draw_batch(2, patch)
        seen_perm += int((perms != (0, 1, 2)).any())
        seen_rows += int(offsets[-1])
        want_image = X.batch_model(plain["image"].cpu().numpy(), perms, rows, offsets)
        assert np.array_equal(_bits(got["image"]), _bits(want_image))
        moved = np.stack([X.permute_model(ids[n], tuple(int(v) for v in perms[n])) for n in range(2)]).astype(np.int32)
        want, want_mask = LC.model_batch(moved, model_cfg)
        assert torch.equal(got["label"].cpu(), torch.from_numpy(want))
        assert torch.equal(got["label_mask"].cpu(), torch.from_numpy(want_mask).float())
    assert seen_perm and seen_rows
    out = main(["--config", str(path), "--mode", "train"])
    assert out["steps"] == 2 and np.isfinite(out["first_loss"]) and np.isfinite(out["last_loss"])


def test_tutorial_minimal_augmented_as_committed(tmp_path, monkeypatch):
    """`python -m pytorch_connectomics_amd.main --config tutorials/minimal_augmented.yaml --mode train` from the repository root, the file
    as committed (32^3 patches of the golden volumes; only the output directory is overridden): its two steps run, the loss is finite"""
    from pytorch_connectomics_amd.main import main
    monkeypatch.chdir(ROOT)
    out = main(["--config", "tutorials/minimal_augmented.yaml", "--mode", "train", f"save_path={tmp_path / 'out'}"])
    assert out["steps"] == 2 and np.isfinite(out["first_loss"]) and np.isfinite(out["last_loss"])
    assert (tmp_path / "out" / "checkpoints" / "last.ckpt").exists()


def test_binary_label_configuration_is_augmented_too(tmp_path):
    """without label targets the (N, 1, D, H, W) fp32 foreground label moves with the image"""
    from pytorch_connectomics_amd.config import load_config
    from pytorch_connectomics_amd.data import AugmentationPlan
    from pytorch_connectomics_amd.main import train_batches
    from types import SimpleNamespace as NS
    path, lab = _tutorial(tmp_path, "minimal_augmented")
    plain_path, _ = _tutorial(tmp_path, "minimal_augmented", edits=(("enabled: true", "enabled: false"),))
    no_targets = ["data.label_transform.targets=[]"]
    cfg, plain_cfg = (load_config(str(q), mode="train", overrides=no_targets) for q in (path, plain_path))
    module = NS(loss_terms=[{"kwargs": {}}])
    dev = torch.device("cuda", 0)
    got, plain = next(iter(train_batches(cfg, module, dev))), next(iter(train_batches(plain_cfg, module, dev)))
    assert not plain["image"].is_cuda and got["image"].is_cuda and got["label"].shape == (2, 1, 16, 16, 16)
    twin = AugmentationPlan.from_config(cfg.data.augmentation, seed=int(cfg.system.seed))
    perms, rows, offsets = twin.draw_batch(2, (16, 16, 16))
    assert np.array_equal(_bits(got["image"]), _bits(X.batch_model(plain["image"].numpy(), perms, rows, offsets)))
    want = np.stack([X.permute_model(plain["label"].numpy()[n], tuple(int(v) for v in perms[n])) for n in range(2)])
    assert np.array_equal(_bits(got["label"]), _bits(want)) and 0.02 < float(got["label"].mean()) < 0.98

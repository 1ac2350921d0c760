"""CPU checks of the device augmentations' host side (pytorch_connectomics_amd/data/augment.py) and of the numpy model the GPU tests
compare the kernels against (tests/augment_cases.py).  The expected arrays of tests/golden/augment.npz come from the reference's own
code (tests/golden/make_golden_augment.py).  Every comparison is exact: fp32 results are compared as their int32 bits."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import augment_cases as X
from pytorch_connectomics_amd import _native as nat
from pytorch_connectomics_amd.data import AugmentationPlan
from pytorch_connectomics_amd.data import augment as A

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def golden():
    return np.load(ROOT / "tests" / "golden" / "augment.npz")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def test_stored_inputs_are_what_the_seeds_regenerate(golden):
    case = X.PURE_CASES["lost_interpolate"]
    assert same_bits(golden["fn__lost_interpolate__in"], X.make_image(case["shape"], case["seed"]))
    image, _ = X.class_case_arrays("RandLostSectiond", 1, X.CLASS_CASES["RandLostSectiond"][1]["seeds"][0])
    assert same_bits(golden["cls__RandLostSectiond__1__in"], image)


@pytest.mark.parametrize("name", sorted(X.PURE_CASES))
def test_model_equals_the_reference_functions(golden, name):
    """the numpy model on the table of a case == the reference's pure function with the case's parameters, bit for bit"""
    case = X.PURE_CASES[name]
    vol = (X.make_ids if case["ids"] else X.make_image)(case["shape"], case["seed"])
    if case["perm"] is not None:
        got = X.permute_model(vol, case["perm"])
    else:
        A.check_rows(case["rows"], case["shape"][1:])
        got = X.defects_model(vol, case["rows"])
    assert same_bits(got, golden[f"fn__{name}__out"])


def test_pure_cases_cover_what_they_claim(golden):
    changed = [n for n, c in X.PURE_CASES.items() if not same_bits(golden[f"fn__{n}__out"],
                                                                    (X.make_ids if c["ids"] else X.make_image)(c["shape"], c["seed"]))]
    assert set(X.PURE_CASES) - set(changed) == {"permute_0", "rot90_000", "rot90_222", "misalign_too_small"}   # three half turns, one per plane, undo each other
    turns = {X.PURE_CASES[f"rot90_{a}{b}{c}"]["perm"] for a in range(4) for b in range(4) for c in range(4)}
    assert len(turns) == 24                                  # the rotation group of the cube


@pytest.mark.parametrize("cls_name", sorted(X.CLASS_CASES))
def test_plan_draws_equal_the_reference_classes(golden, cls_name):
    """a block seeded like the reference class draws what the class draws: the model on the plan's tables == the class's output, for
    every case and seed (no-op draws, zero selected slices and `num_sections` pairs among them)"""
    total = noop = 0
    for i, case in enumerate(X.CLASS_CASES[cls_name]):
        assert len(case["seeds"]) >= 5
        for seed in case["seeds"]:
            image, label = X.class_case_arrays(cls_name, i, seed)
            plan = X.class_plan(cls_name, i, seed)
            assert plan.enabled and list(plan.blocks) == [case["block"]]
            perm, rows = plan.draw_sample(image.shape[1:])
            A.check_signed_perm(perm, image.shape[1:])
            A.check_rows(rows, image.shape[1:])
            got = X.defects_model(np.ascontiguousarray(X.permute_model(image, perm)), rows)
            assert same_bits(got, golden[f"cls__{cls_name}__{i}__{seed}__out"]), (cls_name, i, seed, perm, rows)
            if label is not None:
                assert not rows
                assert same_bits(X.permute_model(label, perm), golden[f"cls__{cls_name}__{i}__{seed}__label_out"]), (cls_name, i, seed, perm)
            # the generator stands where the class left its own: a draw the class takes after the outcome is decided is taken too,
            # so the next sample of a batch sees what a second call of the class would see
            assert int(plan.blocks[case["block"]].R.randint(2 ** 31 - 1)) == int(golden[f"cls__{cls_name}__{i}__next"][seed % 100]), (cls_name, i, seed)
            total += 1
            noop += perm == A.IDENTITY and not rows
    assert total >= 10 and 0 < noop < total


def test_draws_that_must_be_among_the_cases():
    """`prob` missed, zero selected slices with the block fired, and `num_sections` as a pair drawing every count of its range"""
    plan = X.class_plan("RandSliceDropd", 1, 0)              # prob 1, slice_prob 0.05: fires, usually selects nothing
    empty = sum(not X.class_plan("RandSliceDropd", 1, s).draw_sample((6, 9, 11))[1] for s in X.CLASS_CASES["RandSliceDropd"][1]["seeds"])
    assert plan.blocks["slice_drop"].cfg["prob"] == 1.0 and empty >= 1
    counts = {len(X.class_plan("RandLostSectiond", 1, s).draw_sample((6, 9, 11))[1]) for s in range(40)}
    assert counts == {1, 2, 3, 4}
    counts = {len(X.class_plan("RandMissingSectiond", 1, s).draw_sample((6, 9, 11))[1]) for s in range(40)}
    assert counts == {0, 1, 2, 3}
    missed = [not X.class_plan("RandMissingPartsd", 0, s).draw_sample((6, 9, 11))[1] for s in range(40)]
    assert any(missed) and not all(missed)


def _apply_numpy(vol, steps):
    for kind, arg in steps:
        vol = {"transpose": lambda v, a: np.transpose(v, a), "rot90": lambda v, a: np.rot90(v, a[0], a[1]),
               "flip": lambda v, a: np.flip(v, a)}[kind](vol, arg)
    return vol


def test_composition_equals_numpy_in_build_order_for_all_48():
    """axis_permute, rotate90_all, flip and rotate composed into one signed permutation == np.transpose, np.rot90 and np.flip applied
    in build order; the compositions reach all 48 signed permutations"""
    vol = np.arange(5 ** 3, dtype=np.int32).reshape(5, 5, 5)
    R = np.random.RandomState(11)
    reached = set()
    for _ in range(600):
        p = tuple(int(v) for v in R.permutation(3))
        ks = tuple(int(v) for v in R.randint(0, 4, size=3))
        flips = [a for a in range(3) if R.rand() < 0.5]
        plane = tuple(int(v) for v in R.choice(3, size=2, replace=False))
        k = int(R.randint(0, 4))
        perm = A.compose(A.transpose_perm(p), A.rotate90_all_perm(ks))
        steps = [("transpose", p), ("rot90", (ks[0], (2, 1))), ("rot90", (ks[1], (2, 0))), ("rot90", (ks[2], (1, 0)))]
        for a in flips:
            perm = A.compose(perm, A.flip_perm(a))
            steps.append(("flip", a))
        perm = A.compose(perm, A.rot90_perm(k, plane))
        steps.append(("rot90", (k, plane)))
        assert np.array_equal(X.permute_model(vol, perm), _apply_numpy(vol, steps)), (p, ks, flips, plane, k, perm)
        reached.add(perm)
    assert reached == set(X.ALL_PERMS)
    for perm in X.ALL_PERMS:                                 # the model itself: the index map a signed permutation stands for
        src = [v if v >= 0 else -1 - v for v in perm]
        want = np.transpose(vol, src)
        for a, v in enumerate(perm):
            if v < 0:
                want = np.flip(want, a)
        assert np.array_equal(X.permute_model(vol, perm), want)


def test_geometric_blocks_compose_in_build_order():
    """a plan with all four geometric blocks: its permutation == the four blocks' own draws, replayed from equal seeds, through numpy"""
    cfg = {"axis_permute": {"enabled": True}, "rotate90_all": {"enabled": True}, "flip": {"enabled": True, "prob": 0.5},
           "rotate": {"enabled": True, "prob": 0.8, "spatial_axes": [0, 2]}}
    vol = np.arange(4 ** 3, dtype=np.int32).reshape(4, 4, 4)
    for seed in range(12):
        plan = AugmentationPlan(cfg, seed=seed)
        assert list(plan.blocks) == ["axis_permute", "rotate90_all", "flip", "rotate"] and not plan.image and not plan.defects
        perm, rows = plan.draw_sample((4, 4, 4))
        twin = AugmentationPlan(cfg, seed=seed)
        R = {n: b.R for n, b in twin.blocks.items()}
        want = vol
        assert R["axis_permute"].rand() < 1.0
        want = np.transpose(want, R["axis_permute"].permutation(3))
        assert R["rotate90_all"].rand() < 1.0
        for axes in ((2, 1), (2, 0), (1, 0)):
            want = np.rot90(want, int(R["rotate90_all"].randint(0, 4)), axes)
        for a in (0, 1, 2):
            if R["flip"].rand() < 0.5:
                want = np.flip(want, a)
        if R["rotate"].rand() < 0.8:
            want = np.rot90(want, int(R["rotate"].randint(3)) + 1, (0, 2))
        assert not rows and np.array_equal(X.permute_model(vol, perm), want), (seed, perm)
    flat = AugmentationPlan({"axis_permute": {"enabled": True}, "rotate90_all": {"enabled": True}, "flip": {"enabled": True, "prob": 1.0}})
    assert flat.draw_sample((4, 6, 6))[0] == (-1, -2, -3)     # the cubic-only blocks skip a non-cubic patch, as the classes do


def test_block_order_fill_values_and_the_mutex():
    """image rows come in build order; a slice_drop fill lies before the multiply-add (it is scaled), a missing_section fill after it"""
    cfg = {"slice_drop": {"enabled": True, "prob": 1.0, "slice_prob": 1.0, "spatial_axis": 0, "fill_value": 0.5},
           "intensity": {"enabled": True, "banis_style": True, "mul_add_prob": 1.0, "gaussian_noise_prob": 0.0},
           "missing_section": {"enabled": True, "prob": 1.0, "num_sections": 1, "full_section_prob": 1.0},
           "lost_section": {"enabled": True, "prob": 1.0, "num_sections": 2, "mode": "interpolate"},
           "misalignment": {"enabled": True, "prob": 1.0, "displacement": 2}}
    plan = AugmentationPlan(cfg, seed=3)
    assert list(plan.blocks) == ["slice_drop", "intensity", "lost_section", "misalignment", "missing_section"]
    perm, rows = plan.draw_sample((5, 7, 8))
    kinds = [r[0] for r in rows]
    assert perm == A.IDENTITY and kinds[:6] == [nat.AUG_FILL] * 5 + [nat.AUG_MULADD] and kinds[6:8] == [nat.AUG_COPY_SECTION] * 2
    assert kinds[-1] == nat.AUG_FILL and set(kinds[8:-1]) == {nat.AUG_MOVE} and rows[6][1] == rows[7][1] != 0
    image = X.make_image((1, 5, 7, 8), 1)
    out = X.defects_model(image, rows)
    mul, add = np.array(rows[5][2:4], dtype=np.int32).view(np.float32)
    z = rows[-1][2]
    assert (out[0, z].view(np.int32) == rows[-1][8]).all()                       # drawn after the multiply-add: not scaled
    untouched = [k for k in range(5) if k != z and k not in (rows[6][2], rows[7][2])]
    moved = X.defects_model(image, rows[:6] + rows[8:-1])
    assert untouched and all(same_bits(out[0, k], moved[0, k]) for k in untouched)
    assert same_bits(X.defects_model(image, rows[:6]), np.full_like(image, np.float32(0.5)) * mul + add)      # slice_drop's fill is scaled
    one = AugmentationPlan({**cfg, "defect_mutex": True}, seed=3)
    for _ in range(20):
        _, rows = one.draw_sample((5, 7, 8))
        tail = {r[0] for r in rows[6:]}
        assert len(tail) == 1 and len(rows) > 6              # exactly one of the three defects fired


REFUSALS = [({b: {"enabled": True}}, NotImplementedError, b) for b in A.REFUSED_BLOCKS] + [
    ({"misalignment": {"enabled": True, "rotate_ratio": 0.5}}, NotImplementedError, "rotate_ratio"),
    ({"slice_shift_z": {"enabled": True, "rotate_ratio": 0.1}}, NotImplementedError, "rotate_ratio"),
    ({"intensity": {"enabled": True, "banis_style": True}}, NotImplementedError, "gaussian_noise_prob"),
    ({"intensity": {"enabled": True, "gaussian_noise_prob": 0.0}}, NotImplementedError, "contrast_prob"),
    ({"lost_section": {"enabled": True, "mode": "nearest"}}, ValueError, "lost_section.mode"),
    ({"slice_drop": {"enabled": True, "spatial_axis": "every"}}, ValueError, "slice_drop.spatial_axis"),
    ({"slice_shift": {"enabled": True, "spatial_axis": [1, 3]}}, ValueError, "slice_shift.spatial_axis"),
    ({"slice_shift": {"enabled": True, "spatial_axis": []}}, ValueError, "slice_shift.spatial_axis"),
    ({"missing_section": {"enabled": True, "num_sections": [1, 2, 3]}}, ValueError, "missing_section.num_sections"),
    ({"flip": {"enabled": True, "spatial_axis": [0, 3]}}, ValueError, "spatial_axis"),
    ({"rotate": {"enabled": True, "spatial_axes": [1, 1]}}, ValueError, "spatial_axes"),
    ({"flipp": {"enabled": True}}, ValueError, "unknown data.augmentation block"),
    ({"flip": {"enabled": True, "probability": 0.5}}, ValueError, "unexpected keys"),
]


@pytest.mark.parametrize("cfg, error, names", REFUSALS, ids=[r[2] + str(i) for i, r in enumerate(REFUSALS)])
def test_refusals_at_plan_time(cfg, error, names):
    with pytest.raises(error, match=names) as info:
        AugmentationPlan.from_config(cfg)
    if error is NotImplementedError and names in A.REFUSED_BLOCKS:
        assert all(b in str(info.value) for b in A.BUILT_BLOCKS)       # the message lists what is built
    if error is NotImplementedError:
        disabled = {k: {**v, "enabled": False} for k, v in cfg.items()}
        assert not AugmentationPlan.from_config(disabled).enabled      # a refused block that is off refuses nothing


def test_shape_and_mode_refusals():
    flip = {"flip": {"enabled": True}}
    with pytest.raises(NotImplementedError, match="do_2d"):
        AugmentationPlan.from_config(flip, do_2d=True)
    with pytest.raises(NotImplementedError, match="in_channels 5"):
        AugmentationPlan.from_config(flip, in_channels=5)
    assert AugmentationPlan.from_config(flip, in_channels=4).enabled
    assert not AugmentationPlan.from_config({}, do_2d=True, in_channels=9).enabled        # nothing enabled: nothing refused
    rot = {"rotate": {"enabled": True, "spatial_axes": [1, 2]}}
    with pytest.raises(ValueError, match="unequal sides"):
        AugmentationPlan.from_config(rot, patch_size=(8, 8, 9))
    AugmentationPlan.from_config(rot, patch_size=(5, 8, 8))
    with pytest.raises(ValueError, match="unequal sides"):
        AugmentationPlan.from_config(rot).draw_batch(1, (8, 8, 9))
    with pytest.raises(ValueError, match="signed permutation"):
        A.check_signed_perm((0, 0, 2), (4, 4, 4))
    with pytest.raises(ValueError, match="batch shape would change"):
        A.check_signed_perm((1, 0, 2), (4, 5, 5))
    with pytest.raises(ValueError, match="unknown op kind"):
        A.check_rows([(9,) + (0,) * 9], (4, 4, 4))
    with pytest.raises(ValueError, match="section copy"):
        A.check_rows([A.copy_row(0, 1, 1)], (4, 4, 4))
    with pytest.raises(ValueError, match="fill box"):
        A.check_rows([(nat.AUG_FILL, 0, 0, 5, 0, 4, 0, 4, 0, 0)], (4, 4, 4))
    with pytest.raises(NotImplementedError, match="at most"):
        A.check_rows([A.muladd_row(1.0, 0.0)] * (nat.AUG_MAX_OPS + 1), (4, 4, 4))
    with pytest.raises(NotImplementedError, match="more than one group"):
        A.check_rows([A.copy_row(1, 0, 1), A.copy_row(2, 0, 2)], (4, 4, 4))


def test_disabled_config_has_nothing_to_do_and_draws_nothing():
    for cfg in (None, {}, {"flip": {"enabled": False}, "misalignment": {"enabled": False, "prob": 1.0}, "defect_mutex": True, "profile": "x"},
                {"intensity": {"enabled": True, "gaussian_noise_prob": 0.0, "contrast_prob": 0.0, "shift_intensity_prob": 0.0}}):
        plan = AugmentationPlan.from_config(cfg, seed=5)
        assert not plan.enabled and plan.describe() == "nothing to do" and not plan.blocks
        before = plan.mutex_R.get_state()[1].copy()
        perms, ops, offsets = plan.draw_batch(3, (4, 5, 6))
        assert (perms == A.IDENTITY).all() and ops.shape == (0, nat.AUG_ROW) and not offsets.any()
        assert np.array_equal(before, plan.mutex_R.get_state()[1])
        batch = {"image": torch.zeros(1, 1, 4, 5, 6)}
        assert plan(batch) is batch                          # no device, no launch, the batch itself


def test_defaults_are_the_reference_schemas():
    reference = json.loads((ROOT / "tests" / "golden" / "config_defaults.json").read_text())["data"]["augmentation"]
    for name, values in A.DEFAULTS.items():
        assert values == reference[name], name
    assert set(A.DEFAULTS) | set(A.REFUSED_BLOCKS) | {"defect_mutex"} == set(reference) - {"profile"}


def test_shift_intensity_is_one_rounded_add():
    plan = AugmentationPlan({"intensity": {"enabled": True, "gaussian_noise_prob": 0.0, "contrast_prob": 0.0, "shift_intensity_prob": 1.0,
                                           "shift_intensity_offset": 0.1}}, seed=1)
    twin = np.random.RandomState(plan.blocks["intensity"].R.get_state()[1][0])
    _, rows = plan.draw_sample((3, 4, 5))
    assert twin.rand() < 1.0
    offset = float(twin.uniform(-0.1, 0.1))
    image = X.make_image((1, 3, 4, 5), 2)
    assert len(rows) == 1 and same_bits(X.defects_model(image, rows), image + offset)


def test_abi_queries_and_constants():
    lib = nat.lib()
    assert lib.pytc_augment_tile() == 4096 and nat.AUG_ROW == 10 and nat.ABI_VERSION >= 13
    assert (nat.AUG_FILL, nat.AUG_MOVE, nat.AUG_COPY_SECTION, nat.AUG_MULADD) == (0, 1, 2, 3)
    for row in (A.fill_row([0, 1, 0, 1, 0, 1], 0.5, (2, 2, 2)), A.move_row(0, 0, 1, 1, 1, True), A.copy_row(1, 0, 1), A.muladd_row(1.0, 0.0)):
        assert len(row) == nat.AUG_ROW


def test_sampler_offsets_do_not_depend_on_the_augmentation(monkeypatch):
    """`train_batches` cuts the same patches in the same order with and without enabled blocks: the plan's random states are its own"""
    from types import SimpleNamespace as NS
    from pytorch_connectomics_amd import main as M
    from pytorch_connectomics_amd.config import load_config
    import pytorch_connectomics_amd.data as data_pkg

    seen = {}

    def capture(tag):
        def wrap(batches, plan, device):
            assert plan.enabled
            seen[tag] = batches                              # the sampler itself, before any device work
            return batches
        return wrap
    module = NS(loss_terms=[{"kwargs": {}}])
    out = {}
    for tag, overrides in (("plain", []), ("augmented", ["data.augmentation.flip.enabled=true", "data.augmentation.misalignment.enabled=true",
                                                          "data.augmentation.misalignment.prob=1.0", "data.label_transform.targets=[]"])):
        cfg = load_config(str(ROOT / "tutorials" / "minimal_affinity.yaml"), mode="train",
                          overrides=overrides or ["data.label_transform.targets=[]"])
        cfg.data.train.image = str(ROOT / cfg.data.train.image)
        cfg.data.train.label = str(ROOT / cfg.data.train.label)
        monkeypatch.setattr(data_pkg, "augmented_batches", capture(tag))
        it = M.train_batches(cfg, module, torch.device("cpu"))
        out[tag] = [next(it) for _ in range(3)]
    assert "augmented" in seen and "plain" not in seen
    for a, b in zip(out["plain"], out["augmented"]):
        assert torch.equal(a["image"], b["image"]) and torch.equal(a["label"], b["label"])


def test_synthetic_batches_are_neither_planned_nor_refused(monkeypatch):
    """a `random://` / --demo run never read `data.augmentation` and still does not: a refused block there changes nothing, while the
    same section on a real volume fails before the volume is read"""
    from types import SimpleNamespace as NS
    from pytorch_connectomics_amd import main as M
    from pytorch_connectomics_amd import training
    from pytorch_connectomics_amd.config import load_config
    monkeypatch.setattr(training, "synthetic_batches", lambda *a, **k: "synthetic")
    cfg = load_config(str(ROOT / "tutorials" / "minimal_affinity.yaml"), mode="train", overrides=["data.augmentation.elastic.enabled=true"])
    module = NS(loss_terms=[{"kwargs": {}}])
    assert M.train_batches(cfg, module, torch.device("cpu"), demo=True) == "synthetic"
    cfg.data.train.image = "random://demo"
    assert M.train_batches(cfg, module, torch.device("cpu")) == "synthetic"
    cfg.data.train.image = "no_such_volume.npy"
    with pytest.raises(NotImplementedError, match="elastic"):
        M.train_batches(cfg, module, torch.device("cpu"))

"""Host side of the id-volume connected components: the scipy model of tests/label_cc_cases.py against a brute-force flood fill, the
two keys of the label-transform planner, the postprocessing planner's refusals and no-op cases, and the C ABI's symbols, host queries
and refusals (which return before anything is launched).  No GPU."""
import ctypes as C
import logging
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import label_cc_cases as L
from pytorch_connectomics_amd import _native as nat
from pytorch_connectomics_amd.data import LabelTargetTransform
from pytorch_connectomics_amd.decoding.postprocess import PostprocessPlan, apply_decoding_postprocessing, plan_postprocessing

AFFINITY = {"name": "affinity", "kwargs": {"offsets": ["1-0-0", "0-1-0", "0-0-1", "9-0-0"], "affinity_mode": "deepem"}}


# ------------------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("connectivity", L.CONNECTIVITIES)
@pytest.mark.parametrize("name", L.SMALL_CASES)
def test_model_equals_the_flood_fill(name, connectivity):
    ids = L.CASES[name]()
    labels, count = L.model(ids, connectivity)
    want, k = L.flood(ids, connectivity)
    assert int(count[0]) == k and np.array_equal(labels, want)


def test_cases_say_what_they_claim():
    L.self_check()
    assert len(L.bridge_voxels("face")) == 3 and len(L.bridge_voxels("edge")) == 6 and len(L.bridge_voxels("corner")) == 4
    for kind in L.BRIDGE_CLASSES:
        for _, p, q, _tails in L.bridge_voxels(kind):
            crossed = [a for a in range(3) if p[a] // L.TILE[a] != q[a] // L.TILE[a]]
            assert len(crossed) == L.BRIDGE_CLASSES[kind], "the bridge leaves its tile through a face, an edge or a corner"
    heads = L.rank_block_heads()
    assert heads.size > 2 * L.RANK_BLOCK and (heads.ravel()[L.RANK_BLOCK - 1] != 0) and (heads.ravel()[L.RANK_BLOCK] != 0)


def test_dust_model_is_strict():
    labels = L.model(L.dust_case(5), 6)[0]
    out, kept = L.dust(labels, 5)
    sizes = np.bincount(labels.ravel())
    assert sorted(sizes[1:].tolist()) == [1, 4, 4, 5, 5, 6, 6] and int(kept[0]) == 4
    assert set(np.unique(out).tolist()) == {0} | {l for l in range(1, sizes.size) if sizes[l] >= 5}
    same, all_kept = L.dust(labels, 0)
    assert np.array_equal(same, labels) and int(all_kept[0]) == 7


# ------------------------------------------------------------------------------------------------------------- the label planner
def test_planner_reads_the_relabel_keys():
    plan = LabelTargetTransform.from_config({"targets": [AFFINITY], "relabel_connected_components": True, "relabel_connectivity": 26})
    assert plan.relabel_connected_components is True and plan.relabel_connectivity == 26
    ns = LabelTargetTransform.from_config(NS(targets=[AFFINITY], relabel_connected_components=True))
    assert ns.relabel_connected_components is True and ns.relabel_connectivity == 6
    direct = LabelTargetTransform([AFFINITY], relabel_connected_components=True, relabel_connectivity=18)
    assert direct.relabel_connectivity == 18


@pytest.mark.parametrize("bad", [4, 8, 0, 7, 6.5, "six", True])
def test_planner_refuses_other_connectivities(bad):
    with pytest.raises((ValueError, TypeError), match="relabel_connectivity|invalid literal"):
        LabelTargetTransform.from_config({"targets": [AFFINITY], "relabel_connected_components": True, "relabel_connectivity": bad})
    if not isinstance(bad, str):
        with pytest.raises(ValueError, match="relabel_connectivity"):           # refused when the plan is made, on or off
            LabelTargetTransform([AFFINITY], relabel_connectivity=bad)


def test_plan_without_the_keys_is_todays():
    cfg = {"targets": [AFFINITY, {"name": "binary"}, {"name": "instance_boundary"}], "erosion": 1}
    plain = LabelTargetTransform.from_config(cfg)
    off = LabelTargetTransform.from_config({**cfg, "relabel_connected_components": False, "relabel_connectivity": 26})
    none = LabelTargetTransform.from_config({**cfg, "relabel_connected_components": None, "relabel_connectivity": None})
    assert plain.relabel_connected_components is False and plain.relabel_connectivity == 6
    assert none.relabel_connected_components is False and none.relabel_connectivity == 6
    for other in (off, none, LabelTargetTransform.from_config({**cfg, "relabel_connected_components": True})):
        assert other.describe() == plain.describe() and bytes(other.table) == bytes(plain.table) and other.sources == plain.sources
        assert other.channel_names == plain.channel_names and other.uses_mask == plain.uses_mask and other._steps == plain._steps
    label = torch.zeros((1, 2, 3, 4), dtype=torch.int32)
    assert plain.relabel(label) is label and off.relabel(label) is label, "with the key off the step is the identity: no launch"


# ------------------------------------------------------------------------------------------------------ the postprocessing planner
def _cfg(**post):
    return {"decoding": {"postprocessing": post}}


def test_postprocessing_plans():
    assert plan_postprocessing({}) is None and plan_postprocessing({"decoding": {}}) is None
    assert plan_postprocessing(_cfg(enabled=False, instance_cc3d={"connectivity": 26})) is None
    assert plan_postprocessing(_cfg(instance_cc3d={"connectivity": 26})) is None, "enabled defaults to false"
    assert plan_postprocessing(_cfg(enabled=True)) == PostprocessPlan(None, [])
    assert plan_postprocessing(_cfg(enabled=True, instance_cc3d={})) == PostprocessPlan((6, 0), [])
    assert plan_postprocessing(_cfg(enabled=True, instance_cc3d={"connectivity": 26, "min_size": 50}, output_transpose=[2, 1, 0])) == \
        PostprocessPlan((26, 50), [2, 1, 0])
    ns = NS(decoding=NS(postprocessing=NS(enabled=True, instance_cc3d=NS(connectivity=18), binary=NS(enabled=False), output_transpose=None)))
    assert plan_postprocessing(ns) == PostprocessPlan((18, 0), [])


def test_postprocessing_refusals():
    with pytest.raises(NotImplementedError, match=r"postprocessing\.binary"):
        plan_postprocessing(_cfg(enabled=True, binary={"enabled": True, "median_filter_size": 3}))
    assert plan_postprocessing(_cfg(enabled=False, binary={"enabled": True})) is None, "a disabled block refuses nothing"
    for bad in (4, 8, 27, 6.5, None):
        with pytest.raises(ValueError, match=r"instance_cc3d\.connectivity"):
            plan_postprocessing(_cfg(enabled=True, instance_cc3d={"connectivity": bad}))
    with pytest.raises(ValueError, match=r"instance_cc3d\.min_size"):
        plan_postprocessing(_cfg(enabled=True, instance_cc3d={"min_size": 2.5}))


def test_disabled_postprocessing_returns_its_input():
    ids = np.arange(24, dtype=np.int32).reshape(2, 3, 4)
    for cfg in ({}, {"decoding": {}}, _cfg(enabled=False, instance_cc3d={}), NS(decoding=None)):
        assert apply_decoding_postprocessing(cfg, ids) is ids
    t = torch.from_numpy(ids)
    assert apply_decoding_postprocessing(_cfg(enabled=False), t) is t
    with pytest.raises(RuntimeError, match="no CPU path"):
        apply_decoding_postprocessing(_cfg(enabled=True, instance_cc3d={}), t)
    with pytest.raises(TypeError, match="integer ids"):
        apply_decoding_postprocessing(_cfg(enabled=True, instance_cc3d={}), ids.astype(np.float32))


def test_tutorial_plans():
    from pathlib import Path
    from pytorch_connectomics_amd.config import load_config
    path = Path(__file__).resolve().parents[1] / "tutorials" / "minimal_affinity_postprocess.yaml"
    test_cfg = load_config(path, mode="test")
    plan = plan_postprocessing(test_cfg)
    assert plan is not None and plan.instance_cc3d[0] == 26 and plan.instance_cc3d[1] > 0 and plan.output_transpose == []
    train = LabelTargetTransform.from_config(load_config(path, mode="train").data.label_transform)
    assert train.relabel_connected_components is True and train.relabel_connectivity == 6
    base = load_config(path.with_name("minimal_affinity_eval.yaml"), mode="test")
    assert plan_postprocessing(base) is None
    assert LabelTargetTransform.from_config(base.data.label_transform).relabel_connected_components is False


# --------------------------------------------------------------------------------------------------------------------------- the ABI
def test_abi_symbols_and_host_queries():
    names = {"pytc_label_cc", "pytc_label_cc_dust", "pytc_label_cc_tile", "pytc_label_cc_rank_block", "pytc_label_cc_counts",
             "pytc_label_cc_table"}
    assert names <= set(nat.exported_symbols()) and nat.ABI_VERSION >= 16
    lib = nat.lib()
    assert [lib.pytc_label_cc_tile(a) for a in range(4)] == [lib.pytc_affinity_cc_tile(a) for a in range(4)] == [8, 8, 32, 0]
    block = lib.pytc_label_cc_rank_block()
    assert block == 2048
    assert lib.pytc_label_cc_counts(1, 1) == 1 + 1 + 1 and lib.pytc_label_cc_counts(3, block) == 3 + 1 + 3
    assert lib.pytc_label_cc_counts(3, block + 1) == 4 + 1 + 3 and lib.pytc_label_cc_table(3, 1000) == 3000
    for query in (lib.pytc_label_cc_counts, lib.pytc_label_cc_table):
        assert query(0, 5) == 0 and query(1, 0) == 0 and query(1, 2 ** 31 - 1) == 0 and query(2, 2 ** 30) == 0
        assert query(1, 2 ** 31 - 2) > 0
    assert len(nat.SIGNATURES["pytc_label_cc"][1]) == 12 and len(nat.SIGNATURES["pytc_label_cc_dust"][1]) == 11


def _fake(k):
    """an address that is never read: every refusal below returns before a launch"""
    return C.c_void_p(0x10000000 * (k + 1))


def test_abi_refusals_return_before_any_launch():
    lib = nat.lib()
    bufs = [_fake(k) for k in range(6)]                      # ids, flags, parent, counts, labels, count
    call = lambda connectivity, N, dims, b=bufs: lib.pytc_label_cc(b[0], connectivity, b[1], b[2], b[3], b[4], b[5], N, *dims, None)  # noqa: E731
    for connectivity in (0, 4, 8, 7, 27):
        assert call(connectivity, 1, (4, 4, 4)) == nat.ERR_UNSUPPORTED
        assert b"connectivity" in lib.pytc_last_error()
    assert call(6, 1, (2048, 1024, 1024)) == nat.ERR_UNSUPPORTED and b"31 bits" in lib.pytc_last_error()
    assert call(6, 1, (2 ** 31 - 1, 1, 1)) == nat.ERR_UNSUPPORTED, "2^31 - 1 is kept for the background"
    assert call(6, 2, (1024, 1024, 1024)) == nat.ERR_UNSUPPORTED, "the batch counts"
    assert call(6, 0, (4, 4, 4)) == nat.ERR_INVALID and call(6, 1, (4, 0, 4)) == nat.ERR_INVALID
    assert lib.pytc_label_cc(None, 6, bufs[1], bufs[2], bufs[3], bufs[4], bufs[5], 1, 4, 4, 4, None) == nat.ERR_INVALID
    for i in range(6):
        for j in range(i):
            alias = list(bufs)
            alias[i] = C.c_void_p(alias[j].value)            # the same address: an overlap whatever the sizes, so nothing is launched
            assert call(6, 1, (4, 4, 4), alias) == nat.ERR_INVALID and b"alias" in lib.pytc_last_error(), (i, j)
    d = [_fake(k) for k in range(5)]                         # labels, count, table, out, kept
    dust = lambda min_size, b=d, N=1, dims=(4, 4, 4): lib.pytc_label_cc_dust(b[0], b[1], min_size, b[2], b[3], b[4], N, *dims, None)  # noqa: E731
    assert dust(0) == nat.ERR_INVALID and b"min_size" in lib.pytc_last_error()
    assert dust(3, N=2, dims=(1024, 1024, 1024)) == nat.ERR_UNSUPPORTED
    for i in range(5):
        for j in range(i):
            alias = list(d)
            # the same address overlaps whatever the sizes; out == labels is the in-place form, so that pair is shifted by one voxel
            alias[i] = C.c_void_p(alias[j].value + (4 if (i, j) == (3, 0) else 0))
            assert dust(3, alias) == nat.ERR_INVALID and b"alias" in lib.pytc_last_error(), (i, j)


def test_relabel_without_targets_is_refused(tmp_path):
    """the key acts on the id patch of the device target transform: a configuration that sets it and names no targets is told so
    (before any device work), not trained on unrelabelled labels"""
    from pathlib import Path
    from pytorch_connectomics_amd.config import load_config
    from pytorch_connectomics_amd.main import train_batches
    np.save(tmp_path / "img.npy", np.zeros((8, 8, 8), dtype=np.float32))
    np.save(tmp_path / "lab.npy", np.ones((8, 8, 8), dtype=np.int32))
    cfg = load_config(Path(__file__).resolve().parents[1] / "tutorials" / "minimal_affinity_postprocess.yaml", mode="train")
    cfg.data.train.image, cfg.data.train.label = str(tmp_path / "img.npy"), str(tmp_path / "lab.npy")
    cfg.data.label_transform.targets = []
    with pytest.raises(NotImplementedError, match="relabel_connected_components.*needs data.label_transform.targets"):
        train_batches(cfg, NS(loss_terms=[]), torch.device("cpu"))

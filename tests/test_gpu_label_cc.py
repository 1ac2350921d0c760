"""hip_ops.label_cc on the device (csrc/label_cc_kernels.hip): every case of tests/label_cc_cases.py at connectivity 6, 18 and 26 against
the scipy model, integer for integer with the counts; the dust filter at sizes min_size - 1, min_size and min_size + 1; the batch form
against one call per sample; int64 ids and the refusals."""
import numpy as np
import pytest
import torch

import label_cc_cases as L
from pytorch_connectomics_amd import hip_ops

pytestmark = pytest.mark.gpu

_MODEL = {}


def expected(name, connectivity):
    """the model's (labels, count) of a case, computed once and never changed"""
    key = (name, connectivity)
    if key not in _MODEL:
        labels, count = L.model(L.CASES[name](), connectivity)
        labels.setflags(write=False)
        count.setflags(write=False)
        _MODEL[key] = (labels, count)
    return _MODEL[key]


def test_cases_say_what_they_claim():
    L.self_check()


@pytest.mark.parametrize("connectivity", L.CONNECTIVITIES)
@pytest.mark.parametrize("name", sorted(L.CASES))
def test_kernels_equal_the_model(name, connectivity):
    ids = torch.from_numpy(L.CASES[name]()).cuda()
    want, want_count = expected(name, connectivity)
    labels, count, kept = hip_ops.label_cc(ids, connectivity)
    assert labels.is_cuda and labels.dtype == torch.int32 and labels.shape == ids.shape
    assert count.is_cuda and count.dtype == torch.int32 and count.numel() == (ids.shape[0] if ids.dim() == 4 else 1)
    assert kept is count, "nothing is filtered with min_size 0: no launch, no second tensor"
    assert torch.equal(count.cpu(), torch.from_numpy(want_count.copy()))
    got = labels.cpu()
    assert torch.equal(got, torch.from_numpy(want.copy())), f"{int((got.numpy() != want).sum())} of {want.size} voxels differ"


@pytest.mark.parametrize("connectivity", L.CONNECTIVITIES)
def test_checkerboard_components(connectivity):
    ids = L.checker(L.SHAPES["tile_plus"])
    _, count, _ = hip_ops.label_cc(torch.from_numpy(ids).cuda(), connectivity)
    assert int(count.item()) == (int((ids != 0).sum()) if connectivity == 6 else 1)


@pytest.mark.parametrize("connectivity", L.CONNECTIVITIES)
def test_dust_is_strict_and_keeps_the_numbers(connectivity):
    m = 5
    ids = L.dust_case(m)
    labels_np, count_np = L.model(ids, connectivity)
    sizes = np.bincount(labels_np.ravel())[1:]
    assert sorted(sizes.tolist()) == [1, m - 1, m - 1, m, m, m + 1, m + 1]
    want, want_kept = L.dust(labels_np, m)
    out, count, kept = hip_ops.label_cc(torch.from_numpy(ids).cuda(), connectivity, min_size=m)
    assert torch.equal(count.cpu(), torch.from_numpy(count_np)) and int(kept.item()) == int(want_kept[0]) == 4
    got = out.cpu().numpy()
    assert np.array_equal(got, want)
    survivors = np.unique(got[got > 0])
    assert set(survivors.tolist()) == {int(l) for l in range(1, sizes.size + 1) if sizes[l - 1] >= m}, "survivors keep their numbers"
    assert (got[labels_np > 0][sizes[labels_np[labels_np > 0] - 1] == m - 1] == 0).all()


@pytest.mark.parametrize("min_size", [1, 2, 16, 10 ** 6])
def test_dust_on_a_batch(min_size):
    ids = L.CASES["batch_of_three"]()
    labels_np, _ = L.model(ids, 26)
    want, want_kept = L.dust(labels_np, min_size)
    out, count, kept = hip_ops.label_cc(torch.from_numpy(ids).cuda(), 26, min_size=min_size)
    assert torch.equal(out.cpu(), torch.from_numpy(want)) and torch.equal(kept.cpu(), torch.from_numpy(want_kept))
    assert bool((kept <= count).all())


@pytest.mark.parametrize("name", ["full_two_tiles", "serpentine", "blocky__s7_17_65", "minus_one"])
def test_dust_counts_large_components_exactly(name):
    """the sizes are exact where many lanes of a wave add to one cell: the largest component goes at its size + 1 and stays at its size"""
    ids = L.CASES[name]()
    labels_np, _ = expected(name, 6)
    largest = int(np.bincount(labels_np.ravel())[1:].max())
    for min_size in (largest, largest + 1, max(2, largest // 2)):
        want, want_kept = L.dust(labels_np, min_size)
        out, _, kept = hip_ops.label_cc(torch.from_numpy(ids).cuda(), 6, min_size=min_size)
        assert torch.equal(out.cpu(), torch.from_numpy(want)) and int(kept.item()) == int(want_kept[0]), min_size
    assert int(kept.item()) >= 1


def test_batch_equals_one_call_per_sample():
    ids = torch.from_numpy(L.CASES["batch_of_three"]()).cuda()
    labels, count, _ = hip_ops.label_cc(ids, 18)
    for n in range(ids.shape[0]):
        one, k, _ = hip_ops.label_cc(ids[n], 18)
        assert torch.equal(labels[n], one) and int(count[n].item()) == int(k.item())


def test_int64_ids_and_second_call():
    ids = L.CASES["extreme_ids"]()
    a = hip_ops.label_cc(torch.from_numpy(ids).cuda(), 26)
    b = hip_ops.label_cc(torch.from_numpy(ids.astype(np.int64)).cuda(), 26)
    c = hip_ops.label_cc(torch.from_numpy(ids).cuda(), 26)
    assert torch.equal(a[0], b[0]) and torch.equal(a[0], c[0]) and torch.equal(a[1], b[1])


def test_refusals_name_their_argument():
    ids = torch.zeros((2, 3, 4), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="connectivity"):
        hip_ops.label_cc(ids, 8)
    with pytest.raises(ValueError, match="connectivity"):
        hip_ops.label_cc(ids, 6.5)
    with pytest.raises(ValueError, match="ids"):
        hip_ops.label_cc(ids.float())
    with pytest.raises(ValueError, match="ids"):
        hip_ops.label_cc(ids[0])
    with pytest.raises(ValueError, match="min_size"):
        hip_ops.label_cc(ids, 6, min_size=1.5)
    with pytest.raises(RuntimeError, match="ids"):
        hip_ops.label_cc(ids.cpu())
    big = torch.full((2, 3, 4), 2 ** 31, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="ids span"):
        hip_ops.label_cc(big)

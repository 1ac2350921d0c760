"""The cases of the affinity connected components (csrc/cc_kernels.hip, decoding/affinity_cc.py) and a numpy model of their rules.

The model restates DESIGN.md section 4.38 with array operations and scipy's graph components; tests/test_host_affinity_cc.py pins it
to the reference's own serial kernel through tests/golden/affinity_cc.npz, the GPU tests compare the kernels with it exactly.

    hard[a][v] = aff[channels[a]][v] > threshold          strict, NaN false, the threshold rounded to the array's dtype first
    edge v -- v + unit_a                                  iff v + unit_a lies inside and hard[a][v + edge_offset unit_a]
    foreground                                            iff hard[:, v].any() or v ends an edge
    seed                                                  iff hard[:, v].any(): the reference's flood fill starts only there
    ids                                                   0 background; 1 .. K in raster order of every component's smallest seed
                                                          (with edge_offset 0 that is its smallest voxel; with 1 it need not be)

A case is a function -> dict(aff: CPU torch tensor (C, A0, A1, A2), threshold, edge_offset, channels); every one is seeded.  The cases
of `golden_names()` (at most ~20^3 voxels: the reference kernel is plain Python here) are the ones the fixture stores.
"""
from __future__ import annotations

import numpy as np
import torch

TILE = (8, 8, 32)          # the cc_local tile (pytc_affinity_cc_tile); tests/test_host_affinity_cc.py checks it against the library


# ------------------------------------------------------------------------------------------------------------------------------ model
def round_threshold(threshold: float, dtype: torch.dtype) -> float:
    return float(torch.tensor(float(threshold), dtype=torch.float64).to(dtype))


def hard_of(aff: torch.Tensor, threshold: float, channels=(0, 1, 2)) -> np.ndarray:
    """(3, A0, A1, A2) bool.  float16 / float32 go through numpy's own comparison with the Python scalar; bfloat16, which numpy lacks,
    is widened exactly and compared with the threshold rounded to bfloat16."""
    sel = aff[list(channels)]
    if aff.dtype == torch.bfloat16:
        return sel.float().numpy() > np.float32(round_threshold(threshold, torch.bfloat16))
    return sel.numpy() > threshold


def edges_of(hard: np.ndarray, edge_offset: int):
    """(lo, hi) index arrays of the edges, and the foreground mask."""
    shape = hard.shape[1:]
    idx = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
    fg = hard.any(axis=0)
    los, his = [], []
    for a in range(3):
        n = shape[a]
        if n < 2:
            continue
        lo = np.take(idx, range(0, n - 1), axis=a)
        hi = np.take(idx, range(1, n), axis=a)
        on = np.take(hard[a], range(edge_offset, edge_offset + n - 1), axis=a)
        los.append(lo[on])
        his.append(hi[on])
    lo = np.concatenate(los) if los else np.zeros(0, np.int64)
    hi = np.concatenate(his) if his else np.zeros(0, np.int64)
    fg = fg.copy().reshape(-1)
    fg[lo] = True
    fg[hi] = True
    return lo, hi, fg.reshape(shape)


def model_from_hard(hard: np.ndarray, edge_offset: int):
    """-> (labels int32 (A0, A1, A2), K)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    shape = hard.shape[1:]
    V = int(np.prod(shape))
    lo, hi, fg = edges_of(hard, edge_offset)
    graph = coo_matrix((np.ones(lo.size, dtype=np.int8), (lo, hi)), shape=(V, V))
    _, comp = connected_components(graph, directed=False)
    fgv = np.flatnonzero(fg.reshape(-1))
    seeds = np.flatnonzero(hard.any(axis=0).reshape(-1))
    first = np.full(int(comp.max()) + 1 if V else 0, V, dtype=np.int64)
    np.minimum.at(first, comp[seeds], seeds)                  # the smallest seed of every component (V: a background voxel's own)
    order = np.argsort(first, kind="stable")
    K = int((first < V).sum())
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    labels = np.zeros(V, dtype=np.int32)
    labels[fgv] = rank[comp[fgv]] + 1
    return labels.reshape(shape), K


def model(case: dict):
    return model_from_hard(hard_of(case["aff"], case["threshold"], case["channels"]), case["edge_offset"])


# ------------------------------------------------------------------------------------------------------------------------------ cases
def _from_hard(hard: np.ndarray, edge_offset: int, dtype=torch.float32, seed: int = 0) -> dict:
    """Affinities 0.6 .. 0.95 where `hard`, 0.05 .. 0.4 elsewhere; threshold 0.5."""
    rng = np.random.default_rng(seed)
    u = rng.random(hard.shape, dtype=np.float32)
    aff = np.where(hard, 0.6 + 0.35 * u, 0.05 + 0.35 * u).astype(np.float32)
    return dict(aff=torch.from_numpy(aff).to(dtype), threshold=0.5, edge_offset=edge_offset, channels=(0, 1, 2))


def _random(shape, density: float, edge_offset: int, seed: int, dtype=torch.float32) -> dict:
    rng = np.random.default_rng(seed)
    return _from_hard(rng.random((3,) + tuple(shape)) < density, edge_offset, dtype, seed + 1)


def _path_hard(shape, paths, edge_offset: int) -> np.ndarray:
    """hard that joins exactly the consecutive voxels of every path (a list of (i0, i1, i2) one unit step apart)."""
    hard = np.zeros((3,) + tuple(shape), dtype=bool)
    for path in paths:
        p = np.asarray(path, dtype=np.int64)
        assert p.min() >= 0 and (p.max(axis=0) < np.asarray(shape)).all()
        step = np.diff(p, axis=0)
        assert (np.abs(step).sum(axis=1) == 1).all(), "a path moves one unit step at a time"
        axis = np.abs(step).argmax(axis=1)
        low = np.minimum(p[:-1], p[1:])
        low[np.arange(len(axis)), axis] += edge_offset          # the voxel that stores the edge low -- low + unit
        hard[axis, low[:, 0], low[:, 1], low[:, 2]] = True
    return hard


def _walk(waypoints):
    """unit steps through a list of corner points, each differing from the one before along one axis"""
    out = [tuple(waypoints[0])]
    for q in waypoints[1:]:
        p = np.asarray(out[-1])
        d = np.asarray(q) - p
        assert (d != 0).sum() <= 1, (out[-1], q)
        n = int(np.abs(d).sum())
        for k in range(1, n + 1):
            out.append(tuple(p + (d // max(n, 1)) * k))
    return out


def serpentine(shape, pitch=(4, 2), origin=(0, 0, 0)):
    """rows along axis 2 from origin[2] to its mirror image, joined along axis 1 every pitch[1], planes joined along axis 0 every
    pitch[0]"""
    A0, A1, A2 = shape
    o0, o1, o2 = origin
    pts, x_hi, y_up = [], False, True
    for z in range(o0, A0, pitch[0]):
        ys = list(range(o1, A1, pitch[1]))
        for y in (ys if y_up else ys[::-1]):
            pts.append((z, y, A2 - 1 - o2 if x_hi else o2))
            x_hi = not x_hi
            pts.append((z, y, A2 - 1 - o2 if x_hi else o2))
        y_up = not y_up
    return _walk(pts)


def spiral(shape, pitch=(4, 2, 2)):
    """a rectangular spiral inwards in every pitch[0]-th plane, outwards in the next one, the planes joined where a spiral ends"""
    A0, A1, A2 = shape
    n1, n2 = (A1 - 1) // pitch[1] + 1, (A2 - 1) // pitch[2] + 1
    cells, top, left, bottom, right = [], 0, 0, n1 - 1, n2 - 1
    while top <= bottom and left <= right:
        cells += [(top, j) for j in range(left, right + 1)]
        cells += [(i, right) for i in range(top + 1, bottom + 1)]
        if top < bottom:
            cells += [(bottom, j) for j in range(right - 1, left - 1, -1)]
        if left < right:
            cells += [(i, left) for i in range(bottom - 1, top, -1)]
        top, left, bottom, right = top + 1, left + 1, bottom - 1, right - 1
    pts = []
    for k, z in enumerate(range(0, A0, pitch[0])):
        pts += [(z, i * pitch[1], j * pitch[2]) for i, j in (cells if k % 2 == 0 else cells[::-1])]
    return _walk(pts)


SNAKE_SHAPE = (3 * TILE[0], 3 * TILE[1], 3 * TILE[2])


def _two_snakes(edge_offset):
    # the second snake runs in the rows between the first one's, and starts one plane and one row further in
    a = serpentine(SNAKE_SHAPE, pitch=(4, 4), origin=(0, 0, 0))
    b = serpentine(SNAKE_SHAPE, pitch=(4, 4), origin=(2, 2, 1))
    assert not set(a) & set(b)
    return _from_hard(_path_hard(SNAKE_SHAPE, [b, a], edge_offset), edge_offset, seed=77)


def _only_out_of_bounds(shape, edge_offset):
    hard = np.zeros((3,) + tuple(shape), dtype=bool)
    for a in range(3):
        sl = [slice(None)] * 3
        sl[a] = shape[a] - 1 if edge_offset == 0 else 0       # the plane whose only implied edge leaves the volume
        hard[(a,) + tuple(sl)] = True
    return _from_hard(hard, edge_offset, seed=5)


def _checkerboard(shape, edge_offset):
    z, y, x = np.indices(shape)
    hard = np.zeros((3,) + tuple(shape), dtype=bool)
    hard[2] = (x % 4 == edge_offset) & ((z + y) % 2 == 0)      # pairs (x, x + 1) that touch no other edge
    hard[1] = (y % 4 == 2 + edge_offset) & (x % 4 == 3) & (z % 2 == 1)
    return _from_hard(hard, edge_offset, seed=6)


def _threshold_equal():
    rng = np.random.default_rng(8)
    aff = rng.choice(np.asarray([0.25, 0.5, 0.75], dtype=np.float32), size=(3, 9, 10, 11))
    return dict(aff=torch.from_numpy(aff), threshold=0.5, edge_offset=0, channels=(0, 1, 2))


def _non_finite():
    rng = np.random.default_rng(9)
    aff = rng.random((3, 9, 10, 35), dtype=np.float32)
    pick = rng.random(aff.shape)
    aff[pick < 0.1] = np.nan
    aff[(pick >= 0.1) & (pick < 0.2)] = np.inf
    aff[(pick >= 0.2) & (pick < 0.3)] = -np.inf
    return dict(aff=torch.from_numpy(aff), threshold=0.7, edge_offset=1, channels=(0, 1, 2))


def _rounding(dtype):
    """values around the threshold 0.3, which neither 16-bit format holds: float16 rounds it up to 0.300048828125, bfloat16 to
    0.30078125, and a stored value equal to the rounded threshold is not above it"""
    rng = np.random.default_rng(10)
    t = torch.tensor(0.3, dtype=torch.float64).to(dtype)
    ulp = torch.finfo(dtype).eps / 4                            # the spacing in [0.25, 0.5)
    near = torch.stack([t - 2 * ulp, t - ulp, t, t + ulp, t + 2 * ulp]).to(dtype)
    assert float(t) > 0.3 and near.unique().numel() == 5
    aff = near[torch.from_numpy(rng.integers(0, 5, size=(3, 9, 10, 13)))]
    return dict(aff=aff, threshold=0.3, edge_offset=0, channels=(0, 1, 2))


def _six_channels():
    case = _random((9, 10, 35), 0.3, 1, 40)
    rng = np.random.default_rng(41)
    aff = torch.from_numpy(rng.random((6, 9, 10, 35), dtype=np.float32))
    aff[[5, 3, 4]] = case["aff"]
    return dict(aff=aff, threshold=0.5, edge_offset=1, channels=(5, 3, 4))


def _strided_view():
    """every second channel of a 12-channel tensor: a channel stride of two volumes, read in place"""
    big = torch.from_numpy(np.random.default_rng(42).random((12, 9, 10, 35), dtype=np.float32))
    big[::2][[5, 3, 4]] = _random((9, 10, 35), 0.3, 0, 43)["aff"]
    view = big[::2]
    assert not view.is_contiguous() and view[0].is_contiguous()
    return dict(aff=view, threshold=0.5, edge_offset=0, channels=(5, 3, 4))


def _extent_cases():
    out = {}
    for axis, name in enumerate("zyx"):
        t = TILE[axis]
        for k, n in enumerate((t - 1, t, t + 1, 2 * t + 1)):
            shape = [5, 6, 7]
            shape[axis] = n
            out[f"extent_{name}_{n}"] = (lambda s=tuple(shape), e=(k + axis) % 2, sd=100 + 10 * axis + k: _random(s, 0.4, e, sd))
    return out


CASES = {
    "one_voxel_on": lambda: _from_hard(np.ones((3, 1, 1, 1), dtype=bool), 0),
    "one_voxel_off": lambda: _from_hard(np.zeros((3, 1, 1, 1), dtype=bool), 1),
    "line_x": lambda: _random((1, 1, 75), 0.6, 0, 1),
    "line_z": lambda: _random((19, 1, 1), 0.6, 1, 2),
    **_extent_cases(),
    "w_not_multiple_of_4": lambda: _random((6, 9, 13), 0.3, 0, 3),
    "all_false": lambda: _from_hard(np.zeros((3, 9, 10, 35), dtype=bool), 0),
    "all_true_e0": lambda: _from_hard(np.ones((3, 9, 10, 35), dtype=bool), 0),
    "all_true_e1": lambda: _from_hard(np.ones((3, 9, 10, 35), dtype=bool), 1),
    "only_out_of_bounds_e0": lambda: _only_out_of_bounds((9, 10, 35), 0),
    "only_out_of_bounds_e1": lambda: _only_out_of_bounds((9, 10, 35), 1),
    "checkerboard_e0": lambda: _checkerboard((9, 10, 35), 0),
    "checkerboard_e1": lambda: _checkerboard((9, 10, 35), 1),
    **{f"random_{int(100 * d)}_e{e}": (lambda d=d, e=e: _random((17, 18, 67), d, e, 20 + int(100 * d) + e))
       for d in (0.15, 0.25, 0.6) for e in (0, 1)},
    "serpentine_e0": lambda: _from_hard(_path_hard(SNAKE_SHAPE, [serpentine(SNAKE_SHAPE)], 0), 0, seed=70),
    "serpentine_e1": lambda: _from_hard(_path_hard(SNAKE_SHAPE, [serpentine(SNAKE_SHAPE)], 1), 1, seed=71),
    "spiral_e0": lambda: _from_hard(_path_hard(SNAKE_SHAPE, [spiral(SNAKE_SHAPE)], 0), 0, seed=72),
    "spiral_e1": lambda: _from_hard(_path_hard(SNAKE_SHAPE, [spiral(SNAKE_SHAPE)], 1), 1, seed=73),
    "two_snakes_e0": lambda: _two_snakes(0),
    "two_snakes_e1": lambda: _two_snakes(1),
    "threshold_equals_value": _threshold_equal,
    "non_finite": _non_finite,
    "fp16_threshold_rounds": lambda: _rounding(torch.float16),
    "bf16_threshold_rounds": lambda: _rounding(torch.bfloat16),
    "bf16_random": lambda: _random((9, 10, 35), 0.3, 1, 50, torch.bfloat16),
    "fp16_random": lambda: _random((9, 10, 35), 0.3, 0, 51, torch.float16),
    "six_channels_5_3_4": _six_channels,
    "strided_view_5_3_4": _strided_view,
}

GOLDEN_MAX_VOXELS = 8000            # ~20^3: the reference's serial kernel is plain Python without numba


def golden_names():
    """the cases the fixture stores: every case small enough for the plain-Python reference kernel"""
    return [n for n in sorted(CASES) if int(np.prod(CASES[n]()["aff"].shape[1:])) <= GOLDEN_MAX_VOXELS]

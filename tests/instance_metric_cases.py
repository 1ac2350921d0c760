"""A numpy model of the instance metrics (adapted Rand, VOI, instance matching) and the cases the tests run.

The model builds the contingency table n[g][s] by np.unique on the packed keys gt << 32 | seg and applies the formulas of DESIGN.md
section 4.39, which are the reference's metrics/segmentation_numpy.py written over the sparse table:
  A[g] = sum_s n, Bfull[s] = sum_g n, B1[s] = sum_{g>=1} n;
  S_A = sum_{g>=1} A^2, S_B = sum_{s>=1} B1^2, S_AB = sum_{g,s>=1} n^2, c = sum_{g>=1} n[g][0];
  sumB = int64(S_B) + c / N, sumAB = int64(S_AB) + c / N, precision = sumAB / sumB, recall = sumAB / int64(S_A), are = 1 - 2pr/(p+r);
  split = -(1/N1) sum_{g>=1,s} n log2(n / A[g]), merge = -(1/N1) sum_{g>=1,s} n log2(n / B1[s])   (math.fsum);
  a pair g, s >= 1 passes iff float32(float64(n) / float64(A[g] + Bfull[s] - n)) >= float32(thresh);
  tp = the passing pairs (simple) or the size of their maximum matching (augmenting paths, written here).
FIXTURE: the small label pairs tests/golden/make_golden_instance_metrics.py records the reference on.  GPU_CASES(R, W): the cases of
tests/test_gpu_instance_metrics.py for a lane run of R and a workgroup span of W voxels."""
from __future__ import annotations

import math

import numpy as np

THRESHOLDS = (0.3, 0.5, 0.75)
VOI_FRAC_BITS = 27


# ----------------------------------------------------------------------------------------------------------------------- the model
def pair_table(gt, seg):
    """(g, s, n): the distinct pairs in key order and their counts."""
    keys = (np.asarray(gt).astype(np.int64).ravel() << 32) | np.asarray(seg).astype(np.int64).ravel()
    u, n = np.unique(keys, return_counts=True)
    return u >> 32, u & 0xffffffff, n.astype(np.int64)


def _sum_by(ids, n):
    """ids -> (distinct ids, the sum of n per id, the position of every entry's id)"""
    u, inv = np.unique(ids, return_inverse=True)
    tot = np.zeros(len(u), dtype=np.int64)
    np.add.at(tot, inv, n)
    return u, tot, inv


def model_record(gt, seg) -> dict:
    """The integer record, Python ints, and the VOI pair with what its tolerance needs: `voi_terms` = the number of summed terms of
    either entropy, `voi_abs` = the sum of their absolute values (bits), `fixed_terms` / `fixed_abs` = the same for the x log2 x sums of
    the fixed-point form (pairs with g >= 1, gt ids >= 1, seg ids with B1 > 0)."""
    g, s, n = pair_table(gt, seg)
    gu, A, gi = _sum_by(g, n)
    su, Bfull, si = _sum_by(s, n)
    B1 = np.zeros(len(su), dtype=np.int64)
    np.add.at(B1, si[g >= 1], n[g >= 1])
    fg = g >= 1
    py = lambda v: int(v)                                                               # noqa: E731
    sq = lambda v: sum(int(x) * int(x) for x in v)                                      # noqa: E731 -- exact in Python ints
    rec = dict(N=py(n.sum()), N1=py(n[fg].sum()), S_A=sq(A[gu >= 1]), S_B=sq(B1[su >= 1]), S_AB=sq(n[fg & (s >= 1)]),
               c=py(n[fg & (s == 0)].sum()), n_true=py((gu >= 1).sum()), n_pred=py((su >= 1).sum()), pairs=len(n))
    nf, Af, Bf = n[fg].astype(np.float64), A[gi][fg].astype(np.float64), B1[si][fg].astype(np.float64)
    if rec["N1"]:
        t_split, t_merge = nf * np.log2(nf / Af), nf * np.log2(nf / Bf)
        rec["voi"] = (-math.fsum(t_split) / rec["N1"], -math.fsum(t_merge) / rec["N1"])
        rec["voi_abs"] = (math.fsum(np.abs(t_split)), math.fsum(np.abs(t_merge)))
    else:
        rec["voi"], rec["voi_abs"] = (float("nan"), float("nan")), (0.0, 0.0)
    rec["voi_terms"] = int(fg.sum())
    xlx = lambda v: math.fsum(v[v > 0].astype(np.float64) * np.log2(v[v > 0].astype(np.float64)))   # noqa: E731
    rec["fixed_terms"] = int(fg.sum()) + rec["n_true"] + int((B1 > 0).sum())
    rec["fixed_abs"] = xlx(n[fg]) + xlx(A[gu >= 1]) + xlx(B1)
    return rec


def model_matches(gt, seg, thresh) -> np.ndarray:
    """The (g, s) pairs, both >= 1, that pass the float32 score rule, sorted by g then s: int64 (K, 2)."""
    g, s, n = pair_table(gt, seg)
    _, A, gi = _sum_by(g, n)
    _, Bfull, si = _sum_by(s, n)
    score = (n.astype(np.float64) / (A[gi] + Bfull[si] - n).astype(np.float64)).astype(np.float32)
    keep = (g >= 1) & (s >= 1) & (score >= np.float32(thresh))
    return np.stack([g[keep], s[keep]], axis=1).astype(np.int64).reshape(-1, 2)


def model_adapted_rand(rec):
    """(are, precision, recall) as numpy float64, the reference's expressions on its int64 sums."""
    with np.errstate(all="ignore"):
        c_over_n = np.int64(rec["c"]) / rec["N"]
        sum_b, sum_ab = np.int64(rec["S_B"]) + c_over_n, np.int64(rec["S_AB"]) + c_over_n
        p, r = sum_ab / sum_b, sum_ab / np.int64(rec["S_A"])
        return 1.0 - 2.0 * p * r / (p + r), p, r


def maximum_matching(pairs) -> int:
    """The size of a maximum bipartite matching of the pairs, by augmenting paths (Kuhn)."""
    adj = {}
    for g, s in np.asarray(pairs).reshape(-1, 2).tolist():
        adj.setdefault(g, []).append(s)
    owner = {}

    def augment(g, seen):
        for s in adj[g]:
            if s in seen:
                continue
            seen.add(s)
            if s not in owner or augment(owner[s], seen):
                owner[s] = g
                return True
        return False

    return sum(1 for g in adj if augment(g, set()))


def model_matching(rec, pairs, simple: bool) -> dict:
    """The reference's integers and ratios: tp, fp, fn, n_true, n_pred, precision, recall, accuracy, f1."""
    tp = len(pairs) if simple else maximum_matching(pairs)
    fp, fn = rec["n_pred"] - tp, rec["n_true"] - tp
    return dict(tp=tp, fp=fp, fn=fn, n_true=rec["n_true"], n_pred=rec["n_pred"], precision=tp / (tp + fp) if tp > 0 else 0,
                recall=tp / (tp + fn) if tp > 0 else 0, accuracy=tp / (tp + fp + fn) if tp > 0 else 0,
                f1=(2 * tp) / (2 * tp + fp + fn) if tp > 0 else 0)


def voi_tolerance(rec, value: float, against_reference: bool, which: int) -> float:
    """The bound on |implementation - model| (or - the reference's recorded float64) of one entropy, derived, not tuned.
    The implementation sums round(x log2 x 2^f), f = 27, as integers: half a unit 2^-(f+1) per term (`fixed_terms` of them), plus per
    term two ulp of log2 (2 x 2^-52 relative to the term) and the rounding of the product x log2 x (2^-53): 5 x 2^-53 of `fixed_abs`;
    the final int -> float conversion and the division by N1 round once each: 2 x 2^-53 of the value.  All sums are divided by N1.
    The model's own terms n log2(n / m) carry a division, a log2 (taken as two ulp) and a product: 6 x 2^-53 of `voi_abs`, and fsum
    rounds once.  The reference adds its M float64 terms (of probabilities) one after the other: M 2^-53 sum|t| / N1 on top."""
    if not rec["N1"]:
        return 0.0
    u = 2.0 ** -53
    tol = (rec["fixed_terms"] * 2.0 ** -(VOI_FRAC_BITS + 1) + 5 * u * rec["fixed_abs"] + 6 * u * rec["voi_abs"][which]) / rec["N1"]
    tol += 3 * u * abs(value)
    if against_reference:
        tol += rec["voi_terms"] * u * rec["voi_abs"][which] / rec["N1"]
    return tol


# --------------------------------------------------------------------------------------------------------------------- the fixture
def _blocks(rng, shape, block, ids, zero_every=0):
    """a blocky label volume: every `block`-sized box gets one of `ids` random ids (0 with probability 1 / zero_every)"""
    grid = [-(-n // b) for n, b in zip(shape, block)]
    lab = rng.integers(1, ids + 1, size=grid)
    if zero_every:
        lab[rng.integers(0, zero_every, size=grid) == 0] = 0
    for a, b in enumerate(block):
        lab = np.repeat(lab, b, axis=a)
    return np.ascontiguousarray(lab[tuple(slice(0, n) for n in shape)]).astype(np.int64)


def fixture_cases() -> dict:
    """name -> (gt, seg), int64, at most a few thousand voxels each."""
    rng = np.random.default_rng(20261021)
    out = {}
    base = _blocks(rng, (6, 12, 16), (3, 4, 4), 9, zero_every=4)
    out["identical"] = (base, base.copy())
    split = base.copy()
    split[:, :, 8:][base[:, :, 8:] > 0] += 20                                         # every object cut in two along x
    out["pure_split"] = (base, split)
    out["pure_merge"] = (base, (base > 0).astype(np.int64) * 7)
    out["gt_all_zero"] = (np.zeros_like(base), base)
    out["seg_all_zero"] = (base, np.zeros_like(base))
    hole = base.copy()
    hole[2:4, 3:9, 4:12] = 0
    out["seg_zero_inside_gt"] = (base, hole)
    tie_gt = np.zeros((1, 2, 8), dtype=np.int64)
    tie_seg = np.zeros_like(tie_gt)
    tie_gt[0, 0, :4], tie_seg[0, 0, :2], tie_seg[0, 0, 2:4] = 1, 5, 6               # gt 1 faces two halves: IoU 2 / 4 each, exactly 0.5
    tie_gt[0, 1, :6], tie_seg[0, 1, :6] = 2, 9
    out["tie_at_half"] = (tie_gt, tie_seg)
    gaps = np.array([0, 3, 1000, 70000, 2 ** 20 + 5, 17], dtype=np.int64)
    out["sparse_ids"] = (gaps[_blocks(rng, (5, 10, 12), (2, 5, 3), 5)], gaps[::-1][_blocks(rng, (5, 10, 12), (3, 2, 4), 5)])
    out["no_background"] = (_blocks(rng, (4, 9, 11), (2, 3, 4), 6), _blocks(rng, (4, 9, 11), (2, 2, 3), 8))
    out["one_voxel"] = (np.array([[[4]]], dtype=np.int64), np.array([[[2]]], dtype=np.int64))
    out["one_object_each"] = (np.pad(np.ones((3, 5, 6), dtype=np.int64), 2), np.roll(np.pad(np.ones((3, 5, 6), dtype=np.int64), 2), 1, axis=2))
    out["shifted"] = (base, np.roll(base, 2, axis=2))
    k = 0
    for shape, bg, bs, ids, z in (((7, 11, 13), (3, 4, 5), (2, 3, 4), 6, 3), ((4, 16, 16), (2, 4, 4), (2, 4, 8), 12, 0),
                                  ((9, 9, 9), (3, 3, 3), (3, 3, 3), 4, 2), ((3, 20, 30), (1, 5, 6), (1, 4, 7), 20, 5),
                                  ((8, 8, 32), (4, 4, 8), (2, 4, 16), 7, 4), ((5, 7, 64), (5, 7, 4), (1, 7, 9), 30, 6)):
        for variant in range(2):
            gt = _blocks(rng, shape, bg, ids, zero_every=z)
            seg = _blocks(rng, shape, bs, ids + variant * 3, zero_every=z + variant)
            if variant:                                                             # close to the truth: most objects match
                seg = np.where(rng.random(shape) < 0.12, seg, gt * 2)
            out[f"random_blocks_{k}"] = (gt, seg)
            k += 1
    return out


# ----------------------------------------------------------------------------------------------------------------- the GPU cases
def _line(n, run, rng_seed, ids=5):
    """a line of n voxels in runs of about `run` voxels"""
    rng = np.random.default_rng(rng_seed)
    cuts = np.sort(rng.integers(0, n, size=max(1, n // max(1, run))))
    return (np.searchsorted(cuts, np.arange(n), side="right") % ids).astype(np.int64) + rng.integers(0, 2)


def gpu_cases(R: int, W: int) -> dict:
    """name -> a function returning (gt, seg) numpy arrays (their dtypes are the dtypes on the device)."""
    cases = {"n_1": lambda: (np.array([3], dtype=np.int32), np.array([8], dtype=np.int64))}
    for tag, base in (("lane", R), ("span", W)):
        for n in (base - 1, base, base + 1, 2 * base + 1):
            cases[f"line_{tag}_{n}"] = (lambda n=n: (_line(n, 7, n).astype(np.int32), _line(n, 5, n + 1, ids=9).astype(np.int32)))

    def crossing():
        gt = np.arange(1, 2 * W + 1, dtype=np.int64)
        seg = gt[::-1].copy()
        gt[R - 3:R + 4], seg[R - 3:R + 4] = 1, 1                                       # a run across a lane boundary
        gt[W - 5:W + 9], seg[W - 5:W + 9] = 2, 2                                       # and one across a workgroup boundary
        return gt.astype(np.int32), seg
    cases["runs_cross_lane_and_workgroup"] = crossing
    cases["both_constant"] = lambda: (np.full((24, 64, 96), 3, dtype=np.int32), np.full((24, 64, 96), 5, dtype=np.int32))

    def every_voxel():
        i = np.arange(64 * 96 * 160, dtype=np.int64)
        return (i // 1024 + 1).astype(np.int32).reshape(64, 96, 160), (i % 1024 + 1).astype(np.int32).reshape(64, 96, 160)
    cases["every_voxel_its_own_pair"] = every_voxel
    rng = np.random.default_rng(7)
    blocky = _blocks(rng, (12, 40, 56), (4, 8, 8), 11, zero_every=4)
    cases["gt_all_zero"] = lambda: (np.zeros_like(blocky), blocky)
    cases["seg_all_zero"] = lambda: (blocky, np.zeros_like(blocky))

    def largest_ids():
        top = 2 ** 31 - 2
        gt = np.full((4, 4, 4), top, dtype=np.int64)
        seg = np.full((4, 4, 4), top, dtype=np.int64)
        gt[1], seg[2], seg[3, 0] = top - 1, top - 1, 0
        return gt, seg
    cases["ids_2^31-2"] = largest_ids
    for dg in (np.int32, np.int64):
        for ds in (np.int32, np.int64):
            cases[f"dtypes_{np.dtype(dg).name}_{np.dtype(ds).name}"] = (
                lambda dg=dg, ds=ds: (blocky.astype(dg), np.where(blocky % 3 == 0, blocky + 40, np.roll(blocky, 3, axis=2)).astype(ds)))

    def noise():
        noisy = np.random.default_rng(11)
        return noisy.integers(0, 50, size=(33, 35, 37)).astype(np.int32), noisy.integers(0, 70, size=(33, 35, 37)).astype(np.int64)
    cases["noise_33x35x37"] = noise
    return cases

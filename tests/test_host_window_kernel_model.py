"""The CPU model of the window / volume kernels (tests/window_kernel_model.py) against torch, numpy and its own degenerate cases.
The device kernels are held to this model bit for bit (tests/test_gpu_window_exact.py), the lazy / TTA engines run on it against the
reference's fixtures (tests/test_host_lazy_tta.py): here the model itself is checked, on the CPU."""
import itertools

import numpy as np
import pytest
import torch

from oracle import window_oracle as WO
from pytorch_connectomics_amd import _native as nat
from window_kernel_model import KernelModel as M
from window_kernel_model import LEGAL_VIEWS, legal_views, view_legal
import window_exact_shapes as SH


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def test_there_are_32_view_codes_and_the_rest_are_refused():
    assert len(set(LEGAL_VIEWS)) == 32
    assert legal_views((7, 7, 7)) == list(LEGAL_VIEWS)
    assert legal_views((5, 7, 9)) == list(range(8))
    x = _rand(7, 7, 7, 2)
    for bad in (8 | 16, 8 | 32, 16 | 32, 56, 64):
        assert not view_legal(bad, (7, 7, 7))
        with pytest.raises(ValueError):
            M.to_view(x, bad)
        with pytest.raises(ValueError):
            M.from_view(x, bad)
    for view, roi in ((8, (5, 7, 9)), (16, (5, 8, 8)), (32, (9, 9, 5))):
        with pytest.raises(ValueError):
            M.to_view(_rand(*roi, 1), view)


@pytest.mark.parametrize("view", LEGAL_VIEWS)
def test_view_round_trip(view):
    x = _rand(2, 7, 7, 7, 3, seed=view)
    assert torch.equal(M.from_view(M.to_view(x, view), view), x)
    assert torch.equal(M.to_view(M.from_view(x, view), view), x)


@pytest.mark.parametrize("swap,axes", [(nat.VIEW_SWAP_YX, (1, 2)), (nat.VIEW_SWAP_ZY, (0, 1)), (nat.VIEW_SWAP_ZX, (0, 2))])
def test_swap_views_equal_the_torch_transforms(swap, axes):
    """out[z, y, x] = win[T(F(z, y, x))]: the exchange first, then the flips, as torch states them -- e.g. ZX | FLIP_X of a cube is
    torch.flip(x.transpose(z, x), [x]) (the identity tests/test_gpu_tta.py asserts on the device)"""
    x = _rand(7, 7, 7, 2, seed=swap)
    for flips in range(8):
        dims = [d for d, bit in enumerate((nat.VIEW_FLIP_Z, nat.VIEW_FLIP_Y, nat.VIEW_FLIP_X)) if flips & bit]
        want = x.transpose(*axes)
        want = torch.flip(want, dims) if dims else want
        assert torch.equal(M.to_view(x, swap | flips), want)
    # element statement of the same: out[z, y, x] = win[T(F(z, y, x))]
    view = swap | nat.VIEW_FLIP_X | nat.VIEW_FLIP_Z
    out = M.to_view(x, view)
    for z, y, xx in ((0, 1, 2), (6, 0, 3), (4, 4, 1)):
        f = [6 - z, y, 6 - xx]
        f[axes[0]], f[axes[1]] = f[axes[1]], f[axes[0]]
        assert torch.equal(out[z, y, xx], x[f[0], f[1], f[2]])


@pytest.mark.parametrize("mode,np_mode", [("reflect", "reflect"), ("replicate", "edge"), ("circular", "wrap"), ("constant", "constant")])
def test_gather_equals_numpy_pad_of_the_inner_crop(mode, np_mode):
    vol = np.random.default_rng(1).random((2, 9, 10, 14), dtype=np.float32)
    roi = (4, 6, 8)
    wins = list(itertools.product(*WO.lazy_axis_offsets(vol.shape[1:], roi, 0.5)))
    wins += [(8, 2, 3), (-3, 1, 13), (2, -5, 3), (9, 0, 0), (0, 10, 0), (0, 0, -8)]      # thin crops, long pads, wholly outside
    got = M.gather_windows(torch.from_numpy(vol), wins, roi, pad_mode=mode, cval=0.5).numpy()
    for i, w in enumerate(wins):
        lo = [max(0, w[a]) for a in range(3)]
        hi = [min(vol.shape[1 + a], w[a] + roi[a]) for a in range(3)]
        if any(hi[a] <= lo[a] for a in range(3)):
            assert (got[i] == np.float32(0.5)).all(), w
            continue
        inner = vol[:, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        pads = [(0, 0)] + [(max(0, -w[a]), max(0, w[a] + roi[a] - vol.shape[1 + a])) for a in range(3)]
        m = "edge" if np_mode == "reflect" and min(inner.shape[1:]) <= 1 else np_mode
        ref = np.pad(inner, pads, mode=m, **(dict(constant_values=0.5) if m == "constant" else {}))
        np.testing.assert_array_equal(got[i], np.moveaxis(ref, 0, -1), err_msg=f"window {w}")


def test_gather_bf16_rounds_to_nearest_even():
    vol = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -1.0 - 2.0 ** -8]).view(1, 1, 1, 4)
    got = M.gather_windows(vol, [(0, 0, 0)], (1, 1, 4), out_dtype=torch.bfloat16).float().view(-1)
    assert got.tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0]       # ties to even, above a tie rounds up


def _axis_weights(roi, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(n, generator=g) + 0.25 for n in roi]


def test_blend_round_trip_and_degenerate_maps():
    roi, ext = (5, 8, 8), (11, 17, 17)
    vol = _rand(3, *ext, seed=4)
    starts = list(itertools.product((-2, 3, 7), (0, 8), (-1, 9)))
    ones = [torch.ones(n) for n in roi]
    for view in legal_views(roi):
        win = M.gather_windows(vol, starts, roi, view=view)
        value, weight = torch.zeros_like(vol), torch.zeros(ext)
        M.blend_accumulate(win, starts, value, weight, *ones, view=view, combine=nat.BLEND_PRODUCT, floor_w=0.0)
        assert set(weight.unique().tolist()) <= {0.0, 1.0, 2.0, 3.0, 4.0}
        M.blend_finalize(value, weight, clamp=1e-4)
        covered = weight > 0
        assert bool(covered.any()) and not bool(covered.all())
        assert torch.equal(value[:, covered], vol[:, covered])
        assert torch.equal(value[:, ~covered], torch.zeros_like(value[:, ~covered]))
    # the mapped blend with the identity map and zero shifts is the plain blend; the shifted weight with zero shift its weight
    ws = _axis_weights(roi, 5)
    pred = _rand(len(starts), *roi, 3, seed=6)
    for combine, border in ((nat.BLEND_PRODUCT, None), (nat.BLEND_MIN, (1, 2, 0)), (nat.BLEND_PRODUCT, (1, 2, 0))):
        kw = dict(view=9, combine=combine, floor_w=0.4, border=border)
        v0, w0 = _rand(3, *ext, seed=7), _rand(*ext, seed=8)
        v1, w1, w2 = v0.clone(), w0.clone(), w0.clone()
        M.blend_accumulate(pred, starts, v0, w0, *ws, **kw)
        M.blend_accumulate_mapped(pred, starts, v1, w1, *ws, [0, 1, 2], [(0, 0, 0)] * 3, **kw)
        kw.pop("view")
        M.blend_weight_shifted(starts, roi, w2, *ws, (0, 0, 0), **kw)
        assert torch.equal(v0, v1) and torch.equal(w0, w1) and torch.equal(w0, w2)


def test_window_map_floors_and_border():
    wz, wy, wx = torch.tensor([1e-20, 1.0, 0.5]), torch.tensor([1e-20, 0.25, 1.0, 2.0]), torch.tensor([1e-20, 1.0, 3.0])
    tiny = float(np.float32(1.17549435e-38))
    w = M.window_map(wz, wy, wx, nat.BLEND_PRODUCT, 0.0, None)
    assert float(w[0, 0, 0]) == tiny and float(w[1, 1, 2]) == 0.75
    w = M.window_map(wz, wy, wx, nat.BLEND_PRODUCT, 0.5, None)
    assert float(w[0, 0, 0]) == 0.5 and float(w[1, 1, 1]) == 0.5 and float(w[1, 3, 2]) == 6.0
    w = M.window_map(wz, wy, wx, nat.BLEND_MIN, 0.5, None)                       # no floors in MIN
    assert float(w[0, 1, 1]) == float(np.float32(1e-20)) and float(w[1, 1, 2]) == 0.25
    w = M.window_map(wz, wy, wx, nat.BLEND_PRODUCT, 0.5, (1, 1, 0))             # the border wins over the floors
    assert float(w[0, 1, 1]) == 0.0 and float(w[1, 0, 1]) == 0.0 and float(w[1, 1, 0]) == 0.5 and int((w > 0).sum()) == 1 * 2 * 3
    with pytest.raises(ValueError):
        M.window_map(wz, wy, wx, nat.BLEND_PRODUCT, 0.5, (0, 2, 0))             # half the window
    with pytest.raises(ValueError):
        M.window_map(wz, wy, wx, 2, 0.5, None)


@pytest.mark.parametrize("shift", [(0, 0, 0), (1, 0, 0), (-2, 3, 0), (0, -1, -4), (2, 2, 2), (5, 0, 0), (0, -8, 1), (-4, -7, 7)])
def test_a_shifted_channel_drops_exactly_the_wrapped_face(shift):
    roi, ext = (5, 8, 8), (9, 12, 12)
    want = int(np.prod([max(0, roi[a] - abs(shift[a])) for a in range(3)]))
    pred = torch.ones(1, *roi, 2)
    value = torch.zeros(2, *ext)
    weight = torch.zeros(ext)
    ones = [torch.ones(n) for n in roi]
    M.blend_accumulate_mapped(pred, [(2, 2, 2)], value, weight, *ones, [1, 0], [shift, (0, 0, 0)], floor_w=0.0)
    assert int((value[0] != 0).sum()) == want and int((value[1] != 0).sum()) == 5 * 8 * 8 and int((weight != 0).sum()) == 5 * 8 * 8
    w = torch.zeros(ext)
    M.blend_weight_shifted([(2, 2, 2)], roi, w, *ones, shift, floor_w=0.0)
    assert int((w != 0).sum()) == want
    assert torch.equal(w, value[0])                                            # ones predicted, ones weighted: the same box


def test_elementwise_formulas():
    v, w = torch.tensor([3.0, 3.0, 3.0, 0.0]), torch.tensor([2.0, 0.0, -1.0, float("nan")])
    M.normalize_covered(v, w)
    assert v.tolist() == [1.5, 0.0, 0.0, 0.0]
    acc = torch.tensor([9.0, 9.0])
    M.ensemble_update(acc, torch.tensor([1.0, 2.0]), 0, 1)
    assert acc.tolist() == [1.0, 2.0]
    M.ensemble_update(acc, torch.tensor([2.0, 4.0]), 0, 2)
    assert acc.tolist() == [1.5, 3.0]
    stat, cnt = torch.tensor([1.0, 1.0, 1.0, 1.0]), torch.zeros(4)
    M.ensemble_update_masked(stat, cnt, torch.tensor([5.0, 5.0, 5.0, 5.0]), torch.tensor([1.0, 0.0, -1.0, float("nan")]), 0)
    assert stat.tolist() == [6.0, 1.0, 1.0, 1.0] and cnt.tolist() == [1.0, 0.0, 0.0, 0.0]
    M.ensemble_update_masked(stat, cnt, torch.tensor([0.0, 0.0, 0.0, 0.0]), None, 1)
    assert stat.tolist() == [0.0] * 4 and cnt.tolist() == [2.0, 1.0, 1.0, 1.0]
    out = torch.empty(4)
    M.ensemble_finalize_masked(torch.tensor([6.0, 3.0, 1.0, 1.0]), cnt, out, 0)
    assert out.tolist() == [3.0, 3.0, 1.0, 1.0]
    val = torch.tensor([[1.0, 1.0, 1.0]])
    M.blend_finalize(val, torch.tensor([0.0, 0.5, 4.0]), clamp=0.5)
    assert val.tolist() == [[2.0, 2.0, 0.25]]
    x = torch.tensor([-3.0, 0.999, 1.7, 300.0, -0.5])
    assert M.scale_cast(x, scale=100.0, target="uint8").tolist() == [0, 99, 170, 255, 0]
    assert M.scale_cast(x, scale=100.0, target="int8").tolist() == [-128, 99, 127, 127, -50]
    assert M.scale_cast(x, scale=-1.0, target="int16").tolist() == [-3, 0, 1, 300, 0]           # a scale <= 0 is 1; truncation


@pytest.mark.parametrize("mode", ["zscore", "minmax"])
def test_window_normalize_equals_numpy_two_pass_on_integer_windows(mode):
    rng = np.random.default_rng(3)
    x = np.stack([rng.integers(0, 256, 2000), rng.integers(10, 50, 2000), np.full(2000, 7)]).astype(np.float32)
    got = M.window_normalize(torch.from_numpy(x.copy()), mode=nat.NORM_ZSCORE if mode == "zscore" else nat.NORM_MINMAX).numpy()
    for b in range(3):
        d = x[b].astype(np.float64)
        if mode == "zscore":
            sd = d.std()
            want = (x[b] - np.float32(d.mean())) * np.float32(1.0 / sd) if sd > 1e-8 else x[b]
        else:
            want = (x[b] - np.float32(d.min())) * np.float32(1.0 / (d.max() - d.min())) if d.max() > d.min() else x[b]
        np.testing.assert_array_equal(got[b], want)
    assert np.array_equal(got[2], x[2])                                       # the constant window is left as it is
    got = M.window_normalize(torch.from_numpy(x.copy()), mode=nat.NORM_DIVIDE, divide=255.0, binarize=True, threshold=20.0).numpy()
    np.testing.assert_array_equal(got, (x > 20).astype(np.float32) / np.float32(255.0))
    clip = torch.tensor([[10.0, 200.0], [20.0, 30.0], [0.0, 5.0]])
    got = M.window_normalize(torch.from_numpy(x.copy()), clip=clip).numpy()
    np.testing.assert_array_equal(got, np.clip(x, clip[:, :1].numpy(), clip[:, 1:].numpy()))


def _tables(rng, dims, ext, *, lin=(True, True, True), outside=False):
    i0, i1, f = [], [], []
    for a, n in enumerate(dims):
        p = rng.random(n) * (ext[a] - 1)
        lo = np.floor(p).astype(np.int32)
        hi = np.minimum(lo + 1, ext[a] - 1).astype(np.int32)
        fr = (p - lo).astype(np.float32) if lin[a] else np.zeros(n, np.float32)
        if lin[a]:
            fr = np.where(fr == 0, np.float32(0.5), fr)
        if outside:
            lo[rng.integers(0, n)] = -1
        i0.append(lo); i1.append(hi if lin[a] else lo.copy()); f.append(fr)
    return (torch.from_numpy(np.concatenate(i0)), torch.from_numpy(np.concatenate(i1)), torch.from_numpy(np.concatenate(f)))


def test_resample_region_identity_and_trilinear():
    rng = np.random.default_rng(5)
    box = (rng.random((5, 6, 7, 2)) * 100).astype(np.float32)                   # stored (y, z, x, c)
    strides = (1, 7 * 2, 6 * 7 * 2, 2)
    dims = (6, 5, 7)
    ident = torch.from_numpy(np.concatenate([np.arange(n, dtype=np.int32) for n in dims]))
    raw = torch.from_numpy(box.reshape(-1).view(np.uint8).copy())
    out = M.resample_region(raw, "float32", strides, 2, ident, ident.clone(), torch.zeros(18), dims).numpy()
    np.testing.assert_array_equal(out, box.transpose(3, 1, 0, 2))
    vol = box.transpose(3, 1, 0, 2).astype(np.float64)                          # (c, z, y, x)
    for lin, outside in (((True, True, True), False), ((False, True, False), False), ((True, True, True), True)):
        i0, i1, f = _tables(rng, (9, 8, 10), dims, lin=lin, outside=outside)
        got = M.resample_region(raw, "float32", strides, 2, i0, i1, f, (9, 8, 10)).numpy()
        a0, a1, ff = i0.numpy(), i1.numpy(), f.numpy().astype(np.float64)
        z0, y0, x0 = a0[:9], a0[9:17], a0[17:]
        z1, y1, x1 = a1[:9], a1[9:17], a1[17:]
        fz, fy, fx = ff[:9, None, None], ff[9:17][None, :, None], ff[17:][None, None, :]
        t = lambda zi, yi, xi: vol[np.ix_([0, 1], np.maximum(zi, 0), np.maximum(yi, 0), np.maximum(xi, 0))]   # noqa: E731
        want = ((t(z0, y0, x0) * (1 - fx) + t(z0, y0, x1) * fx) * (1 - fy) + (t(z0, y1, x0) * (1 - fx) + t(z0, y1, x1) * fx) * fy) * (1 - fz) \
            + ((t(z1, y0, x0) * (1 - fx) + t(z1, y0, x1) * fx) * (1 - fy) + (t(z1, y1, x0) * (1 - fx) + t(z1, y1, x1) * fx) * fy) * fz
        out_mask = (z0 < 0)[:, None, None] | (y0 < 0)[None, :, None] | (x0 < 0)[None, None, :]
        want = np.where(out_mask[None], 0.0, want)
        assert outside == bool(out_mask.any())
        assert np.abs(got - want).max() <= 1e-6 * np.abs(vol).max()
        assert (got[:, out_mask] == 0).all()


def test_activations_follow_the_dtype_they_are_given():
    x = _rand(5, 6, 7, seed=9) * 4
    for dt in (torch.float32, torch.float64):
        for cl in (False, True):
            v = (x.permute(1, 2, 0) if cl else x).contiguous().to(dt)
            for act, ref in ((nat.ACT_SIGMOID, lambda t: torch.sigmoid(1.5 * t)), (nat.ACT_TANH, lambda t: torch.tanh(1.5 * t)),
                             (nat.ACT_SOFTMAX, lambda t: torch.softmax(t, -1 if cl else 0))):
                got = v.clone()
                M.channel_activation(got, 1, 4, act, 1.5, channels_last=cl)
                assert got.dtype == dt
                sub = (lambda t: t[..., 1:4]) if cl else (lambda t: t[1:4])
                torch.testing.assert_close(sub(got), ref(sub(v)), rtol=0, atol=1e-6 if dt == torch.float32 else 1e-14)
                keep = [0, 4]
                assert torch.equal(got[..., keep] if cl else got[keep], v[..., keep] if cl else v[keep])


def test_the_gpu_suites_shapes_have_the_properties_it_relies_on():
    assert [s for s, _ in SH.WINDOWS] == [(5, 7, 9), (5, 8, 8), (9, 9, 5), (9, 5, 9), (7, 7, 7)]
    seen = set()
    for roi, swaps in SH.WINDOWS:
        n = roi[0] * roi[1] * roi[2]
        assert n > 256 and n % 256 != 0, roi                                   # more than one workgroup, a ragged last one
        for bit in swaps:
            a, b = nat.VIEW_SWAPS[bit]
            assert roi[a] == roi[b]
        assert len(legal_views(roi)) == 8 * (1 + len(swaps))                  # exactly the swaps the table names are legal
        seen |= set(legal_views(roi))
        ext = SH.volume_of(roi)
        assert all(e % 2 == 1 and 2 * r < e <= 2 * r + 3 for e, r in zip(ext, roi)), (roi, ext)
    assert seen == set(LEGAL_VIEWS)                                            # all 32 codes meet a window they are legal for
    assert SH.volume_of((5, 7, 9)) == (11, 15, 19)
    for roi, _ in SH.WINDOWS:
        ext, starts = SH.volume_of(roi), SH.blend_starts(roi)
        cover = np.zeros(ext, int)
        faces = set()
        for s in starts:
            lo = [max(0, s[a]) for a in range(3)]
            hi = [min(ext[a], s[a] + roi[a]) for a in range(3)]
            cover[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] += 1
            faces |= {(a, "lo") for a in range(3) if s[a] < 0} | {(a, "hi") for a in range(3) if s[a] + roi[a] > ext[a]}
        assert cover.max() >= 4 and cover.min() == 0 and len(faces) == 6, (roi, cover.max(), cover.min(), faces)
    assert SH.STRIDE_N == 8192 * 256 + 3 and SH.FLAT_SIZES == (1, 255, 257, SH.STRIDE_N)
    assert SH.CAST_SIZES == (1, 2, 3, 5, 1022, 1023, 8192 * 1024 + 1)
    assert {n % 4 for n in SH.CAST_SIZES} == {1, 2, 3}                          # every length of the scalar tail
    assert SH.CAST_SIZES[-1] > 8192 * 256 * 4 and SH.CAST_SIZES[-1] % 4 == 1   # the stride loop iterates and ends in a scalar tail
    assert SH.NORM_N == 2 * 8192 + 37 and SH.NORM_N % 8192 != 0 and SH.NORM_N > 8192
    nv, c = SH.ACT_FLAT
    assert c == 7 and (nv * c) % 4 == 0 and nv * c >= 65536 * 256 * 4 + 4 * c   # the flat kernel's stride loop iterates ...
    assert (nv - 4) * c < 65536 * 256 * 4 + 4 * c                              # ... at the smallest such size of whole voxels
    nv, c = SH.ACT_RAGGED
    assert (nv * c) % 4 != 0
    rz, ry, rx = SH.RESAMPLE_SECOND
    assert rz * ry * rx > 300 and (rz * ry * rx) % 256 != 0

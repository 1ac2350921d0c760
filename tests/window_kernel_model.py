"""CPU model of the sliding-window and volume-reader kernels (csrc/window_kernels.hip, csrc/volume_kernels.hip), with the signatures
of `pytorch_connectomics_amd.hip_ops` on CPU tensors.

The kernels compute an index per thread; this model is written with slices, flips, transposes and whole-array arithmetic, so the
two statements of each operation are independent.  Every kernel here that is written with explicit roundings (one fp32 rounding per
multiply / add / divide, one writer per element, windows in stream order) is reproduced BIT FOR BIT by plain fp32 array arithmetic:
tests/test_gpu_window_exact.py holds the device to that.  The activations (device expf / tanhf) are evaluated in the dtype of the
tensor the caller passes (fp32 or fp64) and are compared with a tolerance.

The host tests of the lazy / TTA engines (tests/test_host_lazy_tta.py, tests/test_host_tta_engine.py) run the product's
orchestration on this model against the reference's fixtures; tests/test_host_window_kernel_model.py checks the model itself.
"""
import numpy as np
import torch

from pytorch_connectomics_amd import _native as nat

FLT_MIN = np.float32(1.17549435e-38)
MAX_MAP = 32                                   # channels the mapped blend takes (csrc/window_kernels.hip)
_SWAP_AXES = {nat.VIEW_SWAP_YX: (-3, -2), nat.VIEW_SWAP_ZY: (-4, -3), nat.VIEW_SWAP_ZX: (-4, -2)}       # of (..., z, y, x, C)
_SWAP_MASK = nat.VIEW_SWAP_YX | nat.VIEW_SWAP_ZY | nat.VIEW_SWAP_ZX
_FLIPS = ((-4, nat.VIEW_FLIP_Z), (-3, nat.VIEW_FLIP_Y), (-2, nat.VIEW_FLIP_X))
ST_RANGES = {"uint8": (0.0, 255.0), "int8": (-128.0, 127.0), "uint16": (0.0, 65535.0), "int16": (-32768.0, 32767.0),
             "int32": (-2147483648.0, 2147483520.0)}            # int32: the largest fp32 below 2^31
LEGAL_VIEWS = tuple(f | s for s in (0, nat.VIEW_SWAP_YX, nat.VIEW_SWAP_ZY, nat.VIEW_SWAP_ZX) for f in range(8))


def view_legal(view, roi):
    """at most one swap bit, no unknown bit, and the exchanged window axes have equal length"""
    view = int(view)
    if view & ~63:
        return False
    swaps = view & _SWAP_MASK
    if swaps == 0:
        return True
    if swaps not in _SWAP_AXES:
        return False
    a, b = nat.VIEW_SWAPS[swaps]
    return int(roi[a]) == int(roi[b])


def legal_views(roi):
    return [v for v in LEGAL_VIEWS if view_legal(v, roi)]


def _require_view(view, roi):
    if not view_legal(view, roi):
        raise ValueError(f"view code {view}: at most one SWAP bit, and the exchanged window axes must have equal length (window {tuple(roi)})")


def _np32(t):
    a = t.detach().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    assert a.dtype == np.float32, a.dtype
    return a


def _sigmoid(v):
    one = v.dtype.type(1.0)
    with np.errstate(over="ignore"):
        return one / (one + np.exp(-v))


class KernelModel:
    """hip_ops on the CPU.  In-place operations write into the tensors they are handed, like the kernels."""

    @staticmethod
    def require_device(device, what=""):
        return None

    # ---- views -------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def to_view(win, view):
        """canonical window (..., z, y, x, C) -> the view the network sees: out[z, y, x] = win[T(F(z, y, x))], F = per-axis flips,
        T = the exchange of two axes."""
        _require_view(view, win.shape[-4:-1])
        swaps = int(view) & _SWAP_MASK
        if swaps:
            win = win.transpose(*_SWAP_AXES[swaps])
        dims = [d for d, bit in _FLIPS if view & bit]
        return torch.flip(win, dims) if dims else win

    @staticmethod
    def from_view(pred, view):
        """prediction of a view (..., z, y, x, C) -> canonical window frame (the inverse of `to_view`)."""
        _require_view(view, pred.shape[-4:-1])
        dims = [d for d, bit in _FLIPS if view & bit]
        pred = torch.flip(pred, dims) if dims else pred
        swaps = int(view) & _SWAP_MASK
        return pred.transpose(*_SWAP_AXES[swaps]) if swaps else pred

    # ---- window gather ---------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _pad_source(n, before, after, mode):
        """positions in a crop of n elements that a window axis of before + n + after elements reads (np.pad of the crop: periodic
        when the pad is longer than the crop)"""
        idx = np.arange(n)
        j = np.arange(-before, n + after)
        if mode == "replicate":
            return np.clip(j, 0, n - 1)
        if mode == "reflect":
            period = np.concatenate([idx, idx[-2:0:-1]])              # 0 1 .. n-1 n-2 .. 1
        elif mode == "circular":
            period = idx
        else:
            raise AssertionError(mode)
        return period[np.mod(j, len(period))]

    @classmethod
    def gather_plain(cls, vol, starts, roi, pad_mode="constant", cval=0.0):
        """(C, Z, Y, X) -> (B, *roi, C): every window is its in-volume crop, padded out to the window relative to that crop."""
        mode = {"constant": "constant", "reflect": "reflect", "replicate": "replicate", "edge": "replicate", "circular": "circular"}[str(pad_mode)]
        v = _np32(vol)
        ext = v.shape[1:]
        roi = tuple(int(r) for r in roi)
        out = np.empty((len(starts),) + roi + (v.shape[0],), np.float32)
        for i, s in enumerate(starts):
            s = [int(a) for a in s]
            lo = [max(0, s[a]) for a in range(3)]
            hi = [min(ext[a], s[a] + roi[a]) for a in range(3)]
            n = [hi[a] - lo[a] for a in range(3)]
            if min(n) <= 0:                                           # nothing of the window lies in the volume
                out[i] = np.float32(cval)
                continue
            inner = v[:, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
            before = [lo[a] - s[a] for a in range(3)]
            after = [s[a] + roi[a] - hi[a] for a in range(3)]
            m = "replicate" if mode == "reflect" and min(n) <= 1 else mode
            if m == "constant":
                win = np.full((v.shape[0],) + roi, np.float32(cval), np.float32)
                win[:, before[0]:before[0] + n[0], before[1]:before[1] + n[1], before[2]:before[2] + n[2]] = inner
            else:
                win = inner
                for a in range(3):
                    win = np.take(win, cls._pad_source(n[a], before[a], after[a], m), axis=1 + a)
            out[i] = np.moveaxis(win, 0, -1)
        return torch.from_numpy(out)

    @classmethod
    def gather_windows(cls, vol, starts, roi, *, view=0, pad_mode="constant", cval=0.0, out_dtype=torch.float32, out=None, **_kw):
        _require_view(view, roi)
        got = cls.to_view(cls.gather_plain(vol, starts, roi, pad_mode=pad_mode, cval=cval), view).contiguous()
        if out is not None:
            out.copy_(got.to(out.dtype))                              # bf16: round to nearest even
            return out
        return got.to(out_dtype)

    # ---- blending --------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def window_map(wz, wy, wx, combine, floor_w, border):
        """(rz, ry, rx) fp32 weight of a window position.  PRODUCT: fl(fl(wz*wy)*wx), floored at FLT_MIN, then at floor_w; MIN: the
        smallest factor, no floors; the outer `border` voxels are zero whatever the floors gave."""
        z, y, x = (_np32(t.cpu() if isinstance(t, torch.Tensor) else t) for t in (wz, wy, wx))
        if combine == nat.BLEND_MIN:
            w = np.minimum(np.minimum(z[:, None, None], y[None, :, None]), x[None, None, :])
        elif combine == nat.BLEND_PRODUCT:
            w = (z[:, None, None] * y[None, :, None]) * x[None, None, :]
            w = np.maximum(w, FLT_MIN)
            w = np.maximum(w, np.float32(floor_w))
        else:
            raise ValueError(f"unknown combine {combine}")
        w = np.ascontiguousarray(w, np.float32)
        if border is not None and any(int(b) for b in border):
            bz, by, bx = (int(b) for b in border)
            if min(bz, by, bx) < 0 or 2 * bz >= w.shape[0] or 2 * by >= w.shape[1] or 2 * bx >= w.shape[2]:
                raise ValueError("border mask too large for the window")
            keep = np.zeros(w.shape, bool)
            keep[bz:w.shape[0] - bz, by:w.shape[1] - by, bx:w.shape[2] - bx] = True
            w = np.where(keep, w, np.float32(0.0))
        return torch.from_numpy(w)

    @staticmethod
    def _land(dst, src, start, lo=(0, 0, 0)):
        """dst[start + lo ...] += src, clipped to dst (voxels of a window outside the accumulator are skipped)."""
        ext, size = dst.shape[-3:], src.shape[-3:]
        a = [int(start[i]) + lo[i] for i in range(3)]
        l = [max(0, a[i]) for i in range(3)]
        h = [min(ext[i], a[i] + size[i]) for i in range(3)]
        if any(h[i] <= l[i] for i in range(3)):
            return
        d = tuple(slice(l[i], h[i]) for i in range(3))
        s_ = tuple(slice(l[i] - a[i], h[i] - a[i]) for i in range(3))
        dst[(Ellipsis,) + d] += src[(Ellipsis,) + s_]

    @classmethod
    def blend_accumulate(cls, pred, starts, value, weight, wz, wy, wx, *, view=0, combine=0, floor_w=1e-5, border=None):
        """value = fl(value + fl(pred * w)), weight = fl(weight + w), window after window in list order"""
        assert len(starts) == pred.shape[0]
        _require_view(view, pred.shape[1:4])
        w = cls.window_map(wz, wy, wx, combine, floor_w, border)
        canon = cls.from_view(pred.float(), view)                     # bf16 widens exactly
        for i, s in enumerate(starts):
            cls._land(value, canon[i].permute(3, 0, 1, 2) * w, s)
            if weight is not None:
                cls._land(weight, w, s)

    @classmethod
    def blend_accumulate_mapped(cls, pred, starts, value, weight, wz, wy, wx, chan_src, chan_shift, *, view=0, combine=0, floor_w=1e-5,
                                border=None):
        """output channel d <- canonical prediction channel chan_src[d] displaced by chan_shift[d]: the value predicted at q lands
        at p = q + shift, weighted by the window map at p; p outside the window is dropped.  The weight lands unshifted."""
        assert len(starts) == pred.shape[0]
        Cc = pred.shape[-1]
        if Cc > MAX_MAP:
            raise ValueError(f"blend_accumulate_mapped: C={Cc} must be in [1,{MAX_MAP}]")
        if len(chan_src) != Cc or len(chan_shift) != Cc:
            raise ValueError("channel map must describe every output channel")
        _require_view(view, pred.shape[1:4])
        w = cls.window_map(wz, wy, wx, combine, floor_w, border)
        canon = cls.from_view(pred.float(), view)
        roi = canon.shape[1:4]
        for i, s in enumerate(starts):
            for d, (src, sh) in enumerate(zip(chan_src, chan_shift)):
                q_lo = [max(0, -int(sh[a])) for a in range(3)]
                q_hi = [min(roi[a], roi[a] - int(sh[a])) for a in range(3)]
                if any(q_hi[a] <= q_lo[a] for a in range(3)):
                    continue
                q = tuple(slice(q_lo[a], q_hi[a]) for a in range(3))
                p_lo = [q_lo[a] + int(sh[a]) for a in range(3)]
                pbox = tuple(slice(p_lo[a], p_lo[a] + q_hi[a] - q_lo[a]) for a in range(3))
                cls._land(value[d], canon[i][q + (int(src),)] * w[pbox], s, p_lo)
            if weight is not None:
                cls._land(weight, w, s)

    @classmethod
    def blend_weight_shifted(cls, starts, roi, weight, wz, wy, wx, shift, *, combine=0, floor_w=1e-5, border=None):
        """weight += the window map over the positions p of each window whose source p - shift lies inside the window."""
        w = cls.window_map(wz, wy, wx, combine, floor_w, border)
        p_lo = [max(0, int(shift[a])) for a in range(3)]
        p_hi = [min(int(roi[a]), int(roi[a]) + int(shift[a])) for a in range(3)]
        if any(p_hi[a] <= p_lo[a] for a in range(3)):
            return
        box = tuple(slice(p_lo[a], p_hi[a]) for a in range(3))
        for s in starts:
            cls._land(weight, w[box], s, p_lo)

    # ---- elementwise -----------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def normalize_covered(value, weight):
        """v = w > 0 ? v / w : 0"""
        v, w = value.numpy(), np.broadcast_to(weight.numpy(), value.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            v[...] = np.where(w > 0, v / w, v.dtype.type(0.0))

    @staticmethod
    def blend_finalize(value, weight, clamp=1e-4, act=nat.ACT_NONE):
        """v / max(w, clamp) per channel, then the activation -- in the dtype of `value`"""
        v = value.numpy()
        d = np.maximum(weight.numpy().astype(v.dtype).reshape((1,) + tuple(value.shape[1:])), v.dtype.type(np.float32(clamp)))
        r = v / d
        if act == nat.ACT_SIGMOID:
            r = _sigmoid(r)
        elif act == nat.ACT_TANH:
            r = np.tanh(r)
        elif act != nat.ACT_NONE:
            raise AssertionError(act)
        v[...] = r

    @staticmethod
    def ensemble_update(acc, x, mode, count):
        """running mean a + (v - a) / count, or min / max; the first update (count <= 1) copies"""
        a, v = acc.numpy(), x.numpy()
        if count <= 1:
            a[...] = v
        elif mode == 0:
            a[...] = a + (v - a) / a.dtype.type(count)
        elif mode == 1:
            a[...] = np.fmin(a, v)
        else:
            a[...] = np.fmax(a, v)

    @staticmethod
    def ensemble_update_masked(stat, count, x, cover, mode):
        """only voxels with cover > 0 contribute (a NaN cover skips): mean keeps a running sum, min / max the extreme; `count` the
        number of contributions"""
        s, n, v = stat.numpy(), count.numpy(), x.numpy()
        inside = np.ones(v.shape, bool) if cover is None else cover.numpy() > 0
        new = s + v if mode == 0 else (np.fmin(s, v) if mode == 1 else np.fmax(s, v))
        s[...] = np.where(inside, new, s)
        n[...] = np.where(inside, n + n.dtype.type(1.0), n)

    @staticmethod
    def ensemble_finalize_masked(stat, count, out, mode):
        with np.errstate(divide="ignore", invalid="ignore"):
            out.numpy()[...] = stat.numpy() / count.numpy() if mode == 0 else stat.numpy()

    @staticmethod
    def channel_activation(value, c0, c1, act, scale=1.0, *, channels_last=False):
        """channels [c0, c1) <- act(scale * v) in place, in the dtype of `value`; softmax runs over the group and takes no scale"""
        v = value.numpy()
        sub = v[..., c0:c1] if channels_last else v[c0:c1]
        ch = np.moveaxis(sub, -1 if channels_last else 0, 0)           # a view: channel first
        if act == nat.ACT_SOFTMAX:
            m = ch.max(axis=0)
            e = np.exp(ch - m)
            s = np.zeros(m.shape, v.dtype)
            for c in range(e.shape[0]):                               # channel order
                s = s + e[c]
            ch[...] = e / s
            return
        t = ch * v.dtype.type(np.float32(scale))
        if act == nat.ACT_SIGMOID:
            t = _sigmoid(t)
        elif act == nat.ACT_TANH:
            t = np.tanh(t)
        elif act != nat.ACT_NONE:
            raise AssertionError(act)
        ch[...] = t

    @staticmethod
    def scale_cast(x, *, scale=1.0, target="float32"):
        """cast(clip(x * scale)): fp32 multiply, clip for the integer targets, truncating cast (numpy's astype); a scale <= 0 is 1"""
        sc = np.float32(scale)
        u = _np32(x) * (sc if sc > 0 else np.float32(1.0))
        if target in ST_RANGES:
            lo, hi = ST_RANGES[target]
            u = np.clip(u, np.float32(lo), np.float32(hi))
        elif target not in ("float16", "float32"):
            raise ValueError(f"scale_cast: unsupported target dtype {target!r}")
        with np.errstate(over="ignore"):
            return torch.from_numpy(u.astype(target))

    # ---- volume reader ---------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def window_coefficients(v, mode):
        """(shift, scale) of one prepared window: fp64 statistics with the kernel's formulas, rounded to fp32 once"""
        d = v.astype(np.float64).reshape(-1)
        shift, scale = np.float32(0.0), np.float32(1.0)
        if mode == nat.NORM_ZSCORE:
            n = float(d.size)
            mean = d.sum() / n
            var = max((d * d).sum() / n - mean * mean, 0.0)
            sd = np.sqrt(var)
            if sd > 1e-8:
                shift, scale = np.float32(mean), np.float32(1.0 / sd)
        elif mode == nat.NORM_MINMAX:
            mn, mx = d.min(), d.max()
            if mx > mn:
                shift, scale = np.float32(mn), np.float32(1.0 / (mx - mn))
        return shift, scale

    @classmethod
    def window_normalize(cls, x, *, mode=nat.NORM_NONE, binarize=False, threshold=0.0, divide=1.0, clip=None):
        """x fp32 (B, ...), in place, per window: binarise, clip to clip[b] = (lo, hi), then fl(fl(v - shift) * scale) with the
        window's own (shift, scale), or v / divide"""
        a = _np32(x)
        for b in range(a.shape[0]):
            v = a[b]
            if binarize:
                v = np.where(v > np.float32(threshold), np.float32(1.0), np.float32(0.0))
            if clip is not None:
                lo, hi = _np32(clip)[b]
                v = np.fmin(np.fmax(v, lo), hi)
            if mode == nat.NORM_DIVIDE:
                v = v / np.float32(divide)
            elif mode in (nat.NORM_ZSCORE, nat.NORM_MINMAX):
                shift, scale = cls.window_coefficients(v, mode)
                v = (v - shift) * scale
            a[b] = v
        return x

    @staticmethod
    def resample_region(raw_bytes, raw_dtype, strides_czyx, channels, tab_i0, tab_i1, tab_f, dims_zyx):
        """raw box (any storage dtype, element strides in (c, z, y, x)) -> fp32 (C, nz, ny, nx).  Per output axis the tables give the
        two raw indices and the weight f of the second: nearest where all three f are 0, else separable trilinear in the order
        x, y, z with every product and sum rounded to fp32 and 1 - f formed in fp32; i0 < 0 on any axis gives 0."""
        if raw_dtype not in nat.RAW_DTYPES:
            raise TypeError(f"resample_region: stored dtype {raw_dtype} is not supported")
        nz, ny, nx = (int(v) for v in dims_zyx)
        i0, i1, f = tab_i0.numpy().astype(np.int64), tab_i1.numpy().astype(np.int64), _np32(tab_f)
        cuts = ((0, nz), (nz, nz + ny), (nz + ny, nz + ny + nx))
        (z0, y0, x0), (z1, y1, x1), (fz, fy, fx) = ([t[a:b] for a, b in cuts] for t in (i0, i1, f))
        raw = raw_bytes.numpy().view(raw_dtype)
        ext = [int(max(a.max(), b.max())) + 1 for a, b in ((z0, z1), (y0, y1), (x0, x1))]
        item = raw.itemsize
        box = np.lib.stride_tricks.as_strided(raw, shape=(int(channels), *ext), strides=[int(s) * item for s in strides_czyx], writeable=False)
        box = box.astype(np.float32)                                 # (float)v of every storage dtype
        outside = (z0 < 0)[:, None, None] | (y0 < 0)[None, :, None] | (x0 < 0)[None, None, :]

        def tap(zi, yi, xi):
            return box[np.ix_(np.arange(int(channels)), np.maximum(zi, 0), np.maximum(yi, 0), np.maximum(xi, 0))]

        one = np.float32(1.0)
        gx, gy, gz = fx[None, None, None, :], fy[None, None, :, None], fz[None, :, None, None]
        with np.errstate(invalid="ignore", over="ignore"):
            r00 = tap(z0, y0, x0) * (one - gx) + tap(z0, y0, x1) * gx
            r01 = tap(z0, y1, x0) * (one - gx) + tap(z0, y1, x1) * gx
            r10 = tap(z1, y0, x0) * (one - gx) + tap(z1, y0, x1) * gx
            r11 = tap(z1, y1, x0) * (one - gx) + tap(z1, y1, x1) * gx
            q0 = r00 * (one - gy) + r01 * gy
            q1 = r10 * (one - gy) + r11 * gy
            tri = q0 * (one - gz) + q1 * gz
        lin = (fz != 0)[:, None, None] | (fy != 0)[None, :, None] | (fx != 0)[None, None, :]
        out = np.where(lin[None], tri, tap(z0, y0, x0))
        out = np.where(outside[None], np.float32(0.0), out).astype(np.float32)
        return torch.from_numpy(np.ascontiguousarray(out))

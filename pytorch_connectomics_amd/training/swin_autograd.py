"""Autograd Functions of the MONAI SwinUNETR path (models/architectures/swin_unetr.py): window partition / reverse, shifted-window
attention with its relative-position bias table, the 2x2x2 space-to-depth of the patch embedding and of PatchMerging, and LayerNorm at
any width (with or without affine parameters), each forward and backward one or a few HIP kernels (csrc/swin_kernels.hip,
csrc/transformer_kernels.hip).  Linear layers use transformer_autograd.LinearFn as they are.

Token activations are (rows, C) matrices in the compute dtype; parameters stay fp32 and are read as fp32.  Every gradient is a
fixed-order sum (the bias-table gradient included): no atomics, so a training step is bit-reproducible run to run.
"""
from __future__ import annotations

import torch

from .. import hip_ops as ops
from .transformer_autograd import _like, _patch_weight_image, _w


class WindowPartitionFn(torch.autograd.Function):
    """(B * D * H * W, C) tokens -> (B * nW * n, C) window rows: zero pad at the far end of each axis, roll by -shift, partition.
    Backward: the reverse gather (pad rows carry no gradient)."""

    @staticmethod
    def forward(ctx, x, B: int, grid, window, shift):
        ctx.meta = (B, tuple(grid), tuple(window), tuple(shift))
        return ops.window_partition(x.contiguous(), B, grid, window, shift)

    @staticmethod
    def backward(ctx, dw):
        B, grid, window, shift = ctx.meta
        return ops.window_reverse(dw.contiguous(), B, grid, window, shift), None, None, None, None


class WindowReverseFn(torch.autograd.Function):
    """Window rows -> tokens: roll by +shift, crop, + res (the block's residual; None for none).  Backward: the partition gather for
    the window rows, dy itself for the residual."""

    @staticmethod
    def forward(ctx, w, res, B: int, grid, window, shift):
        ctx.meta = (B, tuple(grid), tuple(window), tuple(shift), res is not None)
        if res is not None and res.dtype != w.dtype:
            res = res.to(w.dtype)
        return ops.window_reverse(w.contiguous(), B, grid, window, shift, None if res is None else res.contiguous())

    @staticmethod
    def backward(ctx, dy):
        B, grid, window, shift, has_res = ctx.meta
        dy = dy.contiguous()
        dw = ops.window_partition(dy, B, grid, window, shift) if ctx.needs_input_grad[0] else None
        return dw, dy if has_res and ctx.needs_input_grad[1] else None, None, None, None, None


class WindowAttentionFn(torch.autograd.Function):
    """MONAI WindowAttention on the qkv matrix of window rows (nwin * n, 3 h) -> (nwin * n, h): softmax(q k^T d^-0.5 + bias + mask) v,
    bias = table[relative_position_index[:n, :n]] (MONAI's literal slice of the 7^3 index), mask -100 across shift regions when any
    shift > 0.  Backward: dqkv and the table gradient (a fixed-order sum over every window of the batch)."""

    @staticmethod
    def forward(ctx, qkv, table, nwin: int, heads: int, geom):
        d = int(qkv.shape[1]) // 3 // heads
        scale = float(d) ** -0.5
        t = _w(table)
        out, lse = ops.window_attention_fwd(qkv, t, geom, nwin, heads, scale)
        ctx.save_for_backward(qkv, out, lse, table)
        ctx.meta = (t, nwin, heads, scale, tuple(geom))
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, table = ctx.saved_tensors
        t, nwin, heads, scale, geom = ctx.meta
        dqkv, dt = ops.window_attention_bwd(qkv, t, geom, out, dout.contiguous().to(qkv.dtype), lse, nwin, heads, scale,
                                            want_table=ctx.needs_input_grad[1])
        return dqkv, _like(dt, table), None, None, None


class SpaceToDepth2Fn(torch.autograd.Function):
    """Channels-last (B, D, H, W, C) -> (B * D/2 * H/2 * W/2, 8 C); order 1 is MONAI PatchMerging v1's x0..x7 concatenation (offsets
    (0,1,0) and (0,0,1) twice, (1,1,0) and (0,1,1) never: their gradient is exactly zero).  Backward: the fixed-order scatter-add."""

    @staticmethod
    def forward(ctx, x, order: int):
        ctx.meta = (tuple(x.shape), int(order))
        return ops.space_to_depth2(x.contiguous(), order)

    @staticmethod
    def backward(ctx, dcols):
        shape, order = ctx.meta
        return ops.space_to_depth2_bwd(dcols.contiguous(), shape, order), None


class PatchEmbed2Fn(torch.autograd.Function):
    """MONAI PatchEmbed (Conv3d(C_in, fs, k 2, s 2), no norm) on channels-last x -> (B * D/2 * H/2 * W/2, fs) tokens: the 2^3 cells in
    the conv's tap order times the weight permuted once per weight version to (fs, kd, kh, kw, C_in) columns."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        w2 = _patch_weight_image(weight)
        cols = ops.space_to_depth2(x.contiguous(), 0)
        y = ops.linear_fwd(cols, w2, _w(bias))
        ctx.save_for_backward(cols, weight)
        ctx.meta = (w2, tuple(x.shape))
        return y

    @staticmethod
    def backward(ctx, dy):
        cols, weight = ctx.saved_tensors
        w2, xshape = ctx.meta
        dy = dy.contiguous().to(cols.dtype)
        need = ctx.needs_input_grad
        dc, dW, db, _ = ops.linear_bwd(dy, cols, w2, want_dx=need[0], want_w=need[1], want_b=need[2])
        dx = ops.space_to_depth2_bwd(dc, xshape, 0) if dc is not None else None
        if dW is not None:
            dW = dW.reshape(dW.shape[0], 2, 2, 2, xshape[-1]).permute(0, 4, 1, 2, 3).contiguous()
        return dx, _like(dW, weight), db


class LayerNormRowsFn(torch.autograd.Function):
    """nn.LayerNorm / F.layer_norm over the last axis of a (rows, C) matrix at any C that is a multiple of 16 up to 6144, gamma and
    beta both given or both None (MONAI's proj_out).  Affine widths that are multiples of 64 up to 1024 take pytc_layernorm_wide
    (transformer_autograd.LayerNormFn's kernel); every other case pytc_layernorm_any."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps: float):
        C = int(x.shape[-1])
        wide = gamma is not None and C % 64 == 0 and C <= 1024
        g, b = _w(gamma), _w(beta)
        ctx.save_for_backward(x, gamma)
        ctx.meta = (float(eps), g, wide)
        return ops.layernorm_wide(x, g, b, eps) if wide else ops.layernorm_any(x, g, b, eps)

    @staticmethod
    def backward(ctx, dy):
        x, gamma = ctx.saved_tensors
        eps, g, wide = ctx.meta
        dy = dy.contiguous().to(x.dtype)
        want = gamma is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        if wide:
            dx, dg, db = ops.layernorm_wide_bwd(dy, x, g, eps, want_params=want)
        else:
            dx, dg, db = ops.layernorm_any_bwd(dy, x, g, eps, want_params=want)
        if gamma is None:
            return dx, None, None, None
        return dx, _like(dg, gamma), _like(db, gamma), None


__all__ = ["WindowPartitionFn", "WindowReverseFn", "WindowAttentionFn", "SpaceToDepth2Fn", "PatchEmbed2Fn", "LayerNormRowsFn"]

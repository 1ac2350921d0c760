"""Autograd Functions of the MONAI UNETR path (models/architectures/unetr.py): the ViT encoder and the decoder's k2/s2 transposed
convs, each forward and backward one or a few HIP kernels (csrc/transformer_kernels.hip, csrc/upcat_kernels.hip).

Token activations are (B * N, h) matrices in the compute dtype (bf16 or fp32); weights stay fp32 parameters and are read as fp32 by
the kernels.  Every gradient is a fixed-order sum: no atomics, so a training step is bit-reproducible run to run.
"""
from __future__ import annotations

import torch

from .. import hip_ops as ops


def _w(p):
    return None if p is None else p.detach().float().contiguous()


def _like(g, p):
    return None if g is None else g.to(p.dtype).reshape(p.shape)


# The conv patch embedding's weight (h, C, 16, 16, 16) in the perceptron's (p1 p2 p3 c) column order, rebuilt only when the parameter
# changed (an optimizer step bumps its version): id(weight) -> (weak reference, version, data_ptr, image)
_PATCH_IMAGES: dict = {}


def _patch_weight_image(weight: torch.Tensor) -> torch.Tensor:
    import weakref
    hit = _PATCH_IMAGES.get(id(weight))
    if hit is not None and hit[0]() is weight and hit[1] == weight._version and hit[2] == weight.data_ptr():
        return hit[3]
    img = weight.detach().float().permute(0, 2, 3, 4, 1).reshape(int(weight.shape[0]), -1).contiguous()
    key = id(weight)
    _PATCH_IMAGES[key] = (weakref.ref(weight, lambda _r, _k=key: _PATCH_IMAGES.pop(_k, None)), weight._version, weight.data_ptr(), img)
    return img


class PatchEmbedFn(torch.autograd.Function):
    """tokens = patches(x) . W^T + bias + position_embeddings, broadcast over the batch (MONAI PatchEmbeddingBlock).  x is channels-last
    (B, D, H, W, C_in); `conv` takes the Conv3d(k 16, s 16) weight (h, C_in, 16, 16, 16), permuted once to the (p1 p2 p3 c) column order
    of the perceptron's Linear weight (h, 4096 C_in), once per weight version.  Backward: dW = dY^T . patches, db and dpos fixed-order sums; dx only when x
    requires grad (the scatter of dY . W)."""

    @staticmethod
    def forward(ctx, x, weight, bias, pos, conv: bool):
        h = int(weight.shape[0])
        w2 = _patch_weight_image(weight) if conv else _w(weight)
        patches = ops.patch_gather16(x.contiguous())
        n_tok = int(pos.shape[-2])
        y = ops.linear_fwd(patches, w2, _w(bias), pos.detach().float().reshape(n_tok, h).contiguous())
        ctx.save_for_backward(patches, weight)
        ctx.meta = (conv, w2, tuple(x.shape), n_tok)
        return y

    @staticmethod
    def backward(ctx, dy):
        patches, weight = ctx.saved_tensors
        conv, w2, xshape, n_tok = ctx.meta
        dy = dy.contiguous().to(patches.dtype)
        need = ctx.needs_input_grad
        dp, dW, db, dpos = ops.linear_bwd(dy, patches, w2, want_dx=need[0], want_w=need[1], want_b=need[2],
                                          pos_rows=n_tok if need[3] else 0)
        dx = ops.patch_scatter16(dp, xshape) if dp is not None else None
        if dW is not None and conv:
            C = xshape[-1]
            dW = dW.reshape(dW.shape[0], 16, 16, 16, C).permute(0, 4, 1, 2, 3).contiguous()
        return dx, _like(dW, weight), db, None if dpos is None else dpos.reshape(1, n_tok, -1), None


class LayerNormFn(torch.autograd.Function):
    """nn.LayerNorm over the hidden axis of a (rows, h) token matrix, h a multiple of 64 up to 1024 (pytc_layernorm_wide)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps: float):
        g = _w(gamma)
        ctx.save_for_backward(x, gamma)
        ctx.meta = (float(eps), g)
        return ops.layernorm_wide(x, g, _w(beta), eps)

    @staticmethod
    def backward(ctx, dy):
        x, gamma = ctx.saved_tensors
        eps, g = ctx.meta
        dx, dg, db = ops.layernorm_wide_bwd(dy.contiguous().to(x.dtype), x, g, eps, want_params=ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        return dx, _like(dg, gamma), _like(db, gamma), None


class LinearFn(torch.autograd.Function):
    """y = f(x) . W^T + bias [+ res] on a (rows, K) token matrix, f = GELU when x_gelu -- the qkv, out_proj + residual, linear1 and
    GELU + linear2 + residual layers of a MONAI TransformerBlock.  linear1 stores its pre-activation and linear2 applies the GELU as it
    loads it (the prologue of the pointwise MFMA GEMM), so the backward has the pre-activation for dA = (dY W) * gelu'(A) without a
    second copy.  bf16 with C_in % 64 == 0 and C_out % 128 == 0 (every layer at the default widths) runs on the MFMA GEMM and its
    weight-gradient kernel (ops.linear_mfma_applies); other shapes and fp32 on pytc_linear_*.  The residual's gradient is dY."""

    @staticmethod
    def forward(ctx, x, weight, bias, res, x_gelu: bool):
        w = _w(weight)
        y = ops.linear_fwd(x, w, _w(bias), res=res, x_gelu=x_gelu)
        ctx.save_for_backward(x, weight)
        ctx.meta = (w, bias is not None, res is not None, x_gelu)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        w, has_b, has_res, x_gelu = ctx.meta
        dy = dy.contiguous().to(x.dtype)
        need = ctx.needs_input_grad
        dx, dW, db, _ = ops.linear_bwd(dy, x, w, want_dx=need[0], want_w=need[1], want_b=has_b and need[2], x_gelu=x_gelu)
        return dx, _like(dW, weight), None if db is None else db, dy if (has_res and need[3]) else None, None


class AttentionFn(torch.autograd.Function):
    """Multi-head self-attention of MONAI's SABlock on the qkv GEMM output: (B * N, 3 h) -> (B * N, h), softmax scale d^-0.5.
    Backward recomputes P from Q, K and the saved log-sum-exp; dQ / dK / dV land in the qkv column layout, no atomics."""

    @staticmethod
    def forward(ctx, qkv, B: int, heads: int):
        d = int(qkv.shape[1]) // 3 // heads
        scale = float(d) ** -0.5
        out, lse = ops.attention_fwd(qkv, B, heads, scale)
        ctx.save_for_backward(qkv, out, lse)
        ctx.meta = (B, heads, scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        B, heads, scale = ctx.meta
        return ops.attention_bwd(qkv, out, dout.contiguous().to(qkv.dtype), lse, B, heads, scale), None, None


class Deconv2Fn(torch.autograd.Function):
    """ConvTranspose3d(k 2, s 2, p 0, no bias) on channels-last x, optionally written into the front of a [up, skip] concat buffer
    (MONAI UnetrUpBlock: torch.cat((transp_conv(inp), skip), 1)) -- skip None is the plain deconv of UnetrPrUpBlock.  The
    GEMM-with-scatter-epilogue of csrc/upcat_kernels.hip with the up half at channel offset 0; split-K fixed-order weight gradient."""

    @staticmethod
    def forward(ctx, x_low, weight, skip):
        x_low = x_low.contiguous()
        if skip is not None:
            skip = skip.contiguous() if skip.dtype == x_low.dtype else skip.to(x_low.dtype).contiguous()
        out = ops.deconv2_upfirst_fwd(x_low, _w(weight), skip)
        ctx.save_for_backward(x_low, weight)
        ctx.meta = (0 if skip is None else int(skip.shape[-1]),)
        return out

    @staticmethod
    def backward(ctx, dout):
        x_low, weight = ctx.saved_tensors
        (C_e,) = ctx.meta
        dout = dout.contiguous().to(x_low.dtype)
        need = ctx.needs_input_grad
        dx_e, dx_low, dW, _ = ops.deconv2_upfirst_bwd(dout, x_low, _w(weight), C_e, want_dx_e=C_e > 0 and need[2],
                                                      want_dx_low=need[0], want_w=need[1])
        return dx_low, _like(dW, weight), dx_e


__all__ = ["PatchEmbedFn", "LayerNormFn", "LinearFn", "AttentionFn", "Deconv2Fn"]

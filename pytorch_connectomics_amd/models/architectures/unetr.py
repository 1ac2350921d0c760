"""MONAI UNETR on the MI355X -- counterpart of the `monai_unetr` architecture of the reference
(connectomics/models/architectures/monai_models.py: build_unetr :253-294), which delegates the network to the third-party, un-vendored
`monai` package (monai.networks.nets.UNETR of MONAI 1.3, the last release that takes the `pos_embed=` keyword the reference passes).

The module tree restates that published architecture with the SAME child names, so state-dict keys interchange (unpinned against
MONAI: the package is not part of this engine's environment):

    vit.patch_embedding      position_embeddings (1, n_patches, h); perceptron: patch_embeddings.1 = Linear(16^3 C_in, h) over
                             patch vectors in (p1 p2 p3 c) order; conv: patch_embeddings = Conv3d(C_in, h, k 16, s 16)
    vit.blocks.i (12)        x + attn(norm1 x), then + mlp(norm2 x); attn.qkv Linear(h, 3h, no bias, columns (qkv, head, d)),
                             attn.out_proj, mlp.linear1 -> GELU (erf) -> mlp.linear2; LayerNorm eps 1e-5, softmax scale d^-0.5
    vit.norm                 final LayerNorm
    encoder1                 UnetrBasicBlock = UnetResBlock(C_in -> fs)
    encoder2 / 3 / 4         UnetrPrUpBlock(h -> 2fs / 4fs / 8fs, 2 / 1 / 0 extra (deconv k2 s2, UnetResBlock) stages) on the
                             hidden states of blocks 3 / 6 / 9
    decoder5 / 4 / 3 / 2     UnetrUpBlock: deconv k2 s2 -> cat([up, skip]) -> UnetResBlock(2c -> c)
    out                      UnetOutBlock = 1x1x1 conv with bias
    UnetResBlock             lrelu(norm2(conv2(lrelu(norm1(conv1 x)))) + [norm3(conv3 x) | x]), convs without bias, slope 0.01

The torch.nn children are parameter holders.  `unetr_forward` runs every piece as a HIP kernel with its own autograd backward
(training/transformer_autograd.py for the ViT and the k2/s2 deconvs, training/rsunet_autograd.py for the convs, norms and the
residual sum), on channels-last tensors, in training and inference.  Tokens are row-major over (D/16, H/16, W/16), so on the
channels-last layout `proj_feat` is a view of the (B * N, h) token matrix.  No CPU path.
"""
from __future__ import annotations

from typing import Sequence

import torch
import torch.nn as nn

from .base import ConnectomicsModel
from .monai_models import MONAIModelWrapper
from .registry import register_architecture

PATCH = 16
NUM_LAYERS = 12
ATTENTION_HEAD_DIMS = (32, 64)      # head widths of the attention kernels (pytc_attention_supported)


def _unetr_norm(name, channels: int) -> nn.Module:
    """monai.networks.layers.utils.get_norm_layer for the two norms the UNETR path has kernels for."""
    n = str(name[0] if isinstance(name, (tuple, list)) else name).lower()
    if n == "instance":
        return nn.InstanceNorm3d(channels)
    if n == "batch":
        return nn.BatchNorm3d(channels)
    raise ValueError(f"Unsupported MONAI norm {name!r} for the MI355X UNETR (instance, batch)")


class _ConvOnly(nn.Sequential):
    """monai.networks.blocks.Convolution with conv_only=True (or no norm / act / dropout): one child named `conv`."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, stride: int = 1, bias: bool = False,
                 transposed: bool = False):
        super().__init__()
        if transposed:
            self.add_module("conv", nn.ConvTranspose3d(in_channels, out_channels, kernel_size, stride=stride, bias=bias))
        else:
            self.add_module("conv", nn.Conv3d(in_channels, out_channels, kernel_size, stride=stride, padding=(kernel_size - 1) // 2,
                                              bias=bias))


class UnetResBlock(nn.Module):
    """monai.networks.blocks.dynunet_block.UnetResBlock (kernel 3, stride 1, LeakyReLU 0.01)."""

    def __init__(self, in_channels: int, out_channels: int, norm_name):
        super().__init__()
        self.conv1 = _ConvOnly(in_channels, out_channels, 3)
        self.conv2 = _ConvOnly(out_channels, out_channels, 3)
        self.lrelu = nn.LeakyReLU(negative_slope=0.01)
        self.norm1 = _unetr_norm(norm_name, out_channels)
        self.norm2 = _unetr_norm(norm_name, out_channels)
        self.downsample = in_channels != out_channels
        if self.downsample:
            self.conv3 = _ConvOnly(in_channels, out_channels, 1)
            self.norm3 = _unetr_norm(norm_name, out_channels)


class UnetrBasicBlock(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, norm_name):
        super().__init__()
        self.layer = UnetResBlock(in_channels, out_channels, norm_name)


class UnetrPrUpBlock(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, num_layer: int, norm_name):
        super().__init__()
        self.transp_conv_init = _ConvOnly(in_channels, out_channels, 2, 2, transposed=True)
        self.blocks = nn.ModuleList([nn.Sequential(_ConvOnly(out_channels, out_channels, 2, 2, transposed=True),
                                                   UnetResBlock(out_channels, out_channels, norm_name)) for _ in range(num_layer)])


class UnetrUpBlock(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, norm_name):
        super().__init__()
        self.transp_conv = _ConvOnly(in_channels, out_channels, 2, 2, transposed=True)
        self.conv_block = UnetResBlock(out_channels + out_channels, out_channels, norm_name)


class UnetOutBlock(nn.Module):
    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.conv = _ConvOnly(in_channels, out_channels, 1, bias=True)


class PatchEmbeddingBlock(nn.Module):
    def __init__(self, in_channels: int, img_size: Sequence[int], hidden_size: int, pos_embed: str):
        super().__init__()
        if pos_embed not in ("perceptron", "conv"):
            raise ValueError(f"monai_unetr: pos_embed {pos_embed!r} is not supported (perceptron, conv)")
        self.pos_embed = pos_embed
        self.n_patches = 1
        for s in img_size:
            self.n_patches *= int(s) // PATCH
        if pos_embed == "conv":
            self.patch_embeddings = nn.Conv3d(in_channels, hidden_size, kernel_size=PATCH, stride=PATCH)
        else:       # Sequential(Rearrange, Linear): the Linear is child 1
            self.patch_embeddings = nn.Sequential(nn.Identity(), nn.Linear(PATCH ** 3 * in_channels, hidden_size))
        self.position_embeddings = nn.Parameter(torch.zeros(1, self.n_patches, hidden_size))
        self.dropout = nn.Dropout(0.0)
        with torch.no_grad():          # MONAI's _init_weights: truncated normal std 0.02, zero bias
            nn.init.trunc_normal_(self.position_embeddings, mean=0.0, std=0.02, a=-2.0, b=2.0)
            if pos_embed == "perceptron":
                nn.init.trunc_normal_(self.patch_embeddings[1].weight, mean=0.0, std=0.02, a=-2.0, b=2.0)
                nn.init.zeros_(self.patch_embeddings[1].bias)


class MLPBlock(nn.Module):
    def __init__(self, hidden_size: int, mlp_dim: int, dropout_rate: float):
        super().__init__()
        self.linear1 = nn.Linear(hidden_size, mlp_dim)
        self.linear2 = nn.Linear(mlp_dim, hidden_size)
        self.fn = nn.GELU()
        self.drop1 = nn.Dropout(dropout_rate)
        self.drop2 = nn.Dropout(dropout_rate)


class SABlock(nn.Module):
    def __init__(self, hidden_size: int, num_heads: int, dropout_rate: float):
        super().__init__()
        self.num_heads = num_heads
        self.out_proj = nn.Linear(hidden_size, hidden_size)
        self.qkv = nn.Linear(hidden_size, hidden_size * 3, bias=False)
        self.drop_output = nn.Dropout(dropout_rate)
        self.drop_weights = nn.Dropout(dropout_rate)
        self.head_dim = hidden_size // num_heads
        self.scale = self.head_dim ** -0.5


class TransformerBlock(nn.Module):
    def __init__(self, hidden_size: int, mlp_dim: int, num_heads: int, dropout_rate: float):
        super().__init__()
        self.mlp = MLPBlock(hidden_size, mlp_dim, dropout_rate)
        self.norm1 = nn.LayerNorm(hidden_size)
        self.attn = SABlock(hidden_size, num_heads, dropout_rate)
        self.norm2 = nn.LayerNorm(hidden_size)


class ViT(nn.Module):
    def __init__(self, in_channels: int, img_size: Sequence[int], hidden_size: int, mlp_dim: int, num_heads: int, pos_embed: str,
                 dropout_rate: float):
        super().__init__()
        self.patch_embedding = PatchEmbeddingBlock(in_channels, img_size, hidden_size, pos_embed)
        self.blocks = nn.ModuleList([TransformerBlock(hidden_size, mlp_dim, num_heads, dropout_rate) for _ in range(NUM_LAYERS)])
        self.norm = nn.LayerNorm(hidden_size)


class UNETR(nn.Module):
    """monai.networks.nets.UNETR (MONAI 1.3; spatial_dims 3, patch 16, 12 layers, qkv_bias False, conv_block = res_block = True,
    classification False) with the same child names, so state-dict keys interchange."""

    def __init__(self, in_channels: int, out_channels: int, img_size: Sequence[int], feature_size: int = 16, hidden_size: int = 768,
                 mlp_dim: int = 3072, num_heads: int = 12, pos_embed: str = "perceptron", norm_name="instance",
                 dropout_rate: float = 0.0):
        super().__init__()
        img_size = tuple(int(s) for s in img_size)
        if len(img_size) == 2:
            raise NotImplementedError("monai_unetr: the MI355X engine builds the 3-D UNETR only (input_size has 2 axes)")
        if len(img_size) != 3:
            raise ValueError(f"monai_unetr: model.input_size must have 3 axes, got {list(img_size)}")
        if not 0 <= dropout_rate <= 1:
            raise ValueError("dropout_rate should be between 0 and 1.")
        if hidden_size % num_heads != 0:
            raise ValueError("hidden_size should be divisible by num_heads.")
        if hidden_size // num_heads not in ATTENTION_HEAD_DIMS:
            raise NotImplementedError(f"monai_unetr: head width hidden_size / num_heads = {hidden_size // num_heads} has no HIP attention "
                                      "kernel (32 or 64)")
        if hidden_size % 64 or hidden_size > 1024:
            raise NotImplementedError(f"monai_unetr: hidden_size {hidden_size} has no HIP LayerNorm kernel (a multiple of 64 up to 1024)")
        bad = [s for s in img_size if s < PATCH or s % PATCH]
        if bad:
            raise ValueError(f"monai_unetr: every axis of model.input_size {list(img_size)} must be a positive multiple of the "
                             f"patch size {PATCH}")
        _unetr_norm(norm_name, 1)        # refuse an unsupported norm before building anything
        self.img_size = img_size
        self.patch_size = (PATCH,) * 3
        self.feat_size = tuple(s // PATCH for s in img_size)
        self.hidden_size, self.num_heads = hidden_size, num_heads
        self.dropout_rate = float(dropout_rate)
        self.num_layers = NUM_LAYERS
        self.classification = False
        fs = feature_size
        self.vit = ViT(in_channels, img_size, hidden_size, mlp_dim, num_heads, pos_embed, dropout_rate)
        self.encoder1 = UnetrBasicBlock(in_channels, fs, norm_name)
        self.encoder2 = UnetrPrUpBlock(hidden_size, fs * 2, 2, norm_name)
        self.encoder3 = UnetrPrUpBlock(hidden_size, fs * 4, 1, norm_name)
        self.encoder4 = UnetrPrUpBlock(hidden_size, fs * 8, 0, norm_name)
        self.decoder5 = UnetrUpBlock(hidden_size, fs * 8, norm_name)
        self.decoder4 = UnetrUpBlock(fs * 8, fs * 4, norm_name)
        self.decoder3 = UnetrUpBlock(fs * 4, fs * 2, norm_name)
        self.decoder2 = UnetrUpBlock(fs * 2, fs, norm_name)
        self.out = UnetOutBlock(fs, out_channels)

    def forward(self, x):  # pragma: no cover - guard only
        raise RuntimeError("the MONAI-style UNETR executes through MONAIModelWrapper.forward (HIP engine); its modules are "
                           "parameter holders")


# ---------------------------------------------------------------------------------------------------- HIP execution
def _norm(n: nn.Module, x: torch.Tensor, slope: float) -> torch.Tensor:
    """norm -> LeakyReLU(slope); slope 1 is the identity (the norms whose activation comes after the residual sum)."""
    from ...training.rsunet_autograd import NormActFn
    if isinstance(n, nn.BatchNorm3d):
        return NormActFn.apply(x, n.weight, n.bias, None, "batch", 1, float(n.eps), "leakyrelu", slope, n)
    return NormActFn.apply(x, None, None, None, "instance", 1, float(n.eps), "leakyrelu", slope, None)


def _conv(m: _ConvOnly, x: torch.Tensor) -> torch.Tensor:
    from ...training.rsunet_autograd import ResampleConv3dFn
    c = m.conv
    return ResampleConv3dFn.apply(x, c.weight, c.bias, 1, int(c.padding[0]), False)


def _res_block(m: UnetResBlock, x: torch.Tensor) -> torch.Tensor:
    from ...training.rsunet_autograd import AddFn, NormActFn
    slope = float(m.lrelu.negative_slope)
    y = _norm(m.norm2, _conv(m.conv2, _norm(m.norm1, _conv(m.conv1, x), slope)), 1.0)
    res = _norm(m.norm3, _conv(m.conv3, x), 1.0) if m.downsample else x
    return NormActFn.apply(AddFn.apply(y, res), None, None, None, "none", 1, 0.0, "leakyrelu", slope, None)


def _deconv(m: _ConvOnly, x: torch.Tensor, skip=None) -> torch.Tensor:
    from ...training.transformer_autograd import Deconv2Fn
    return Deconv2Fn.apply(x, m.conv.weight, skip)


def _pr_up(m: UnetrPrUpBlock, x: torch.Tensor) -> torch.Tensor:
    x = _deconv(m.transp_conv_init, x)
    for blk in m.blocks:
        x = _res_block(blk[1], _deconv(blk[0], x))
    return x


def _up(m: UnetrUpBlock, x: torch.Tensor, skip: torch.Tensor) -> torch.Tensor:
    return _res_block(m.conv_block, _deconv(m.transp_conv, x, skip))


def _vit_block(blk: TransformerBlock, x: torch.Tensor, B: int) -> torch.Tensor:
    from ...training.transformer_autograd import AttentionFn, LayerNormFn, LinearFn
    a = blk.attn
    qkv = LinearFn.apply(LayerNormFn.apply(x, blk.norm1.weight, blk.norm1.bias, blk.norm1.eps), a.qkv.weight, a.qkv.bias, None, False)
    o = AttentionFn.apply(qkv, B, a.num_heads)
    x = LinearFn.apply(o, a.out_proj.weight, a.out_proj.bias, x, False)
    mp = blk.mlp
    a1 = LinearFn.apply(LayerNormFn.apply(x, blk.norm2.weight, blk.norm2.bias, blk.norm2.eps), mp.linear1.weight, mp.linear1.bias,
                        None, False)
    return LinearFn.apply(a1, mp.linear2.weight, mp.linear2.bias, x, True)         # GELU applied to the pre-activation as it is read


def unetr_forward(net: UNETR, x: torch.Tensor) -> torch.Tensor:
    """UNETR on channels-last x (B, D, H, W, C_in) -> (B, D, H, W, C_out); nothing is built lazily or shared between calls (safe on
    the window engine's side streams)."""
    from ...training.transformer_autograd import LayerNormFn, PatchEmbedFn
    if tuple(int(s) for s in x.shape[1:4]) != net.img_size:
        raise ValueError(f"monai_unetr: input spatial size {tuple(int(s) for s in x.shape[1:4])} differs from model.input_size "
                         f"{list(net.img_size)} (the position embedding is fixed to it; sliding windows must equal input_size)")
    if net.training and net.dropout_rate > 0:
        raise NotImplementedError(f"monai_unetr: dropout {net.dropout_rate} > 0 in training mode has no HIP kernel "
                                  "(model.transformer.dropout must be 0.0)")
    B = int(x.shape[0])
    pe = net.vit.patch_embedding
    if pe.pos_embed == "conv":
        w, b = pe.patch_embeddings.weight, pe.patch_embeddings.bias
    else:
        w, b = pe.patch_embeddings[1].weight, pe.patch_embeddings[1].bias
    t = PatchEmbedFn.apply(x, w, b, pe.position_embeddings, pe.pos_embed == "conv")
    grid = (B, *net.feat_size, net.hidden_size)
    hidden = []
    for blk in net.vit.blocks:
        t = _vit_block(blk, t, B)
        hidden.append(t)
    nv = net.vit.norm
    dec4 = LayerNormFn.apply(t, nv.weight, nv.bias, nv.eps).view(grid)      # proj_feat: a view on channels-last
    enc1 = _res_block(net.encoder1.layer, x)
    enc2 = _pr_up(net.encoder2, hidden[3].view(grid))
    enc3 = _pr_up(net.encoder3, hidden[6].view(grid))
    enc4 = _pr_up(net.encoder4, hidden[9].view(grid))
    u = _up(net.decoder5, dec4, enc4)
    u = _up(net.decoder4, u, enc3)
    u = _up(net.decoder3, u, enc2)
    u = _up(net.decoder2, u, enc1)
    return _conv(net.out.conv, u)


@register_architecture("monai_unetr")
def build_unetr(cfg) -> ConnectomicsModel:
    """MONAI UNETR: model.input_size, model.{in,out}_channels, model.transformer.{feature_size 16, hidden_size 768, mlp_dim 3072,
    num_heads 12, pos_embed "perceptron", norm "instance", dropout 0.0} (reference monai_models.py:253-294)."""
    tc = getattr(cfg.model, "transformer", None)
    size = getattr(cfg.model, "input_size", None)
    if not size:
        raise ValueError("monai_unetr needs model.input_size (the ViT's position embedding is fixed to it)")
    model = UNETR(
        in_channels=cfg.model.in_channels, out_channels=cfg.model.out_channels, img_size=list(size),
        feature_size=getattr(tc, "feature_size", 16), hidden_size=getattr(tc, "hidden_size", 768),
        mlp_dim=getattr(tc, "mlp_dim", 3072), num_heads=getattr(tc, "num_heads", 12),
        pos_embed=getattr(tc, "pos_embed", "perceptron"), norm_name=getattr(tc, "norm", "instance"),
        dropout_rate=getattr(tc, "dropout", 0.0))
    return MONAIModelWrapper(model)


__all__ = ["UNETR", "ViT", "PatchEmbeddingBlock", "TransformerBlock", "SABlock", "MLPBlock", "UnetResBlock", "UnetrBasicBlock",
           "UnetrPrUpBlock", "UnetrUpBlock", "UnetOutBlock", "unetr_forward", "build_unetr"]

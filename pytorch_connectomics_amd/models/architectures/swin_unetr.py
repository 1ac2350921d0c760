"""MONAI SwinUNETR on the MI355X -- counterpart of the `monai_swin_unetr` architecture of the reference
(connectomics/models/architectures/monai_models.py: build_swin_unetr :297-334), which delegates the network to the third-party,
un-vendored `monai` package (monai.networks.nets.SwinUNETR of MONAI 1.3: depths (2, 2, 2, 2), heads (3, 6, 12, 24), window 7,
patch 2, mlp_ratio 4, qkv_bias, norm "instance", normalize, downsample "merging" (v1), use_v2 False, spatial_dims 3).

The module tree restates that published architecture with the SAME child names, so state-dict keys interchange (unpinned against
MONAI: the package is not part of this engine's environment):

    swinViT.patch_embed.proj         Conv3d(C_in, fs, k 2, s 2) (patch_norm False: no norm)
    swinViT.layers{1..4}.0           BasicLayer at dim fs 2^(i-1), heads 3 2^(i-1): blocks.{0, 1} (unshifted, shifted) and
                                     downsample = PatchMerging v1 (cat of 8 offsets -> norm LayerNorm(8 dim) -> reduction, no bias)
    SwinTransformerBlock             x + reverse(attn(partition(pad(roll(norm1 x))))), then + mlp(norm2 x); mlp.linear1 -> GELU (erf)
                                     -> mlp.linear2; LayerNorm eps 1e-5
    WindowAttention                  relative_position_bias_table (13^3, heads), relative_position_index (343, 343) persistent buffer,
                                     qkv Linear(dim, 3 dim) with bias, proj; softmax(q k^T d^-0.5 + bias [+ mask]) v
    encoder1 / 2 / 3 / 4 / 10        UnetrBasicBlock = UnetResBlock on the input and on the normalised hidden states 0 / 1 / 2 / 4
    decoder5 / 4 / 3 / 2 / 1         UnetrUpBlock: deconv k2 s2 -> cat([up, skip]) -> UnetResBlock(2c -> c)
    out                              UnetOutBlock = 1x1x1 conv with bias

The torch.nn children are parameter holders.  `swin_unetr_forward` runs every piece as a HIP kernel with its own autograd backward
(training/swin_autograd.py for the window partition / attention / reverse, the 2x2x2 space-to-depth and the LayerNorms,
training/transformer_autograd.py for the linear layers and the k2/s2 deconvs, training/rsunet_autograd.py for the convs, norms and
the residual sum), on channels-last tensors, in training and inference.  Tokens are channels-last rows, so MONAI's
`b c d h w <-> b d h w c` rearranges are no-ops.  No CPU path.

relative_position_index is registered as MONAI registers it, but it is a constant of the architecture (a function of the 7^3 window
alone): the kernels compute its entries, index[i][j] = c13(i) - c13(j) + 1098 with c13(t) = (t / 49) 169 + (t / 7 % 7) 13 + t % 7,
which `relative_position_index()` below equals (tests/test_host_swin_unetr.py).  use_checkpoint is accepted and changes no number; it
saves no memory on this engine either (every activation a backward kernel reads is kept).
"""
from __future__ import annotations

from typing import Sequence

import torch
import torch.nn as nn

from .base import ConnectomicsModel
from .monai_models import MONAIModelWrapper
from .registry import register_architecture
from .unetr import MLPBlock, UnetOutBlock, UnetrBasicBlock, UnetrUpBlock, _conv, _res_block, _unetr_norm, _up

WINDOW = 7
PATCH = 2
DEPTHS = (2, 2, 2, 2)
NUM_HEADS = (3, 6, 12, 24)
MLP_RATIO = 4.0
WINDOW_HEAD_DIMS = (16, 32)          # head widths of the window-attention kernels (pytc_window_attention_supported)
STAGE_FACTOR = PATCH ** 5            # every axis of the input must divide by it


# ---------------------------------------------------------------------------------------------------- host helpers
def get_window_size(x_size: Sequence[int], window_size: Sequence[int], shift_size=None):
    """monai.networks.nets.swin_unetr.get_window_size: on an axis no longer than the window the window shrinks to the axis and the
    shift becomes 0 (that axis only)."""
    use_window = list(window_size)
    use_shift = list(shift_size) if shift_size is not None else None
    for i in range(len(x_size)):
        if x_size[i] <= window_size[i]:
            use_window[i] = x_size[i]
            if use_shift is not None:
                use_shift[i] = 0
    if use_shift is None:
        return tuple(use_window)
    return tuple(use_window), tuple(use_shift)


def relative_position_index(window_size: Sequence[int] = (WINDOW,) * 3) -> torch.Tensor:
    """WindowAttention.relative_position_index of MONAI 1.3 (3-D): (prod(ws), prod(ws)) int64."""
    ws = [int(w) for w in window_size]
    coords = torch.stack(torch.meshgrid(torch.arange(ws[0]), torch.arange(ws[1]), torch.arange(ws[2]), indexing="ij"))
    flat = torch.flatten(coords, 1)
    rel = (flat[:, :, None] - flat[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws[0] - 1
    rel[:, :, 1] += ws[1] - 1
    rel[:, :, 2] += ws[2] - 1
    rel[:, :, 0] *= (2 * ws[1] - 1) * (2 * ws[2] - 1)
    rel[:, :, 1] *= 2 * ws[2] - 1
    return rel.sum(-1)


def sliced_index(n: int) -> torch.Tensor:
    """The index the n-token windows read: MONAI's literal relative_position_index[:n, :n] of the full 7^3 window (for n < 343 not
    the geometric relative position of the smaller window)."""
    return relative_position_index()[:n, :n]


def kernel_index(n: int) -> torch.Tensor:
    """What the attention kernels compute for sliced_index(n): c13(i) - c13(j) + 1098."""
    t = torch.arange(n)
    c13 = (t // 49) * 169 + (t // 7 % 7) * 13 + t % 7
    return c13[:, None] - c13[None, :] + 1098


def _axis_label(p: int, P: int, ws: int, s: int) -> int:
    return 2 if s == 0 else (0 if p < P - ws else (1 if p < P - s else 2))


def mask_region_labels(dims: Sequence[int], window_size: Sequence[int], shift_size: Sequence[int]) -> torch.Tensor:
    """(nW, n) int64 region labels of compute_mask on the padded grid `dims`, windows and tokens in partition order, as the kernels
    compute them: per axis 0 below P - ws, 1 below P - s, else 2 (all 2 when that axis' shift is 0, MONAI's slice(-0, None))."""
    P, ws, s = [int(v) for v in dims], [int(v) for v in window_size], [int(v) for v in shift_size]
    lab = torch.empty(P, dtype=torch.int64)
    for d in range(P[0]):
        for h in range(P[1]):
            for w in range(P[2]):
                lab[d, h, w] = (_axis_label(d, P[0], ws[0], s[0]) * 9 + _axis_label(h, P[1], ws[1], s[1]) * 3
                                + _axis_label(w, P[2], ws[2], s[2]))
    lab = lab.view(P[0] // ws[0], ws[0], P[1] // ws[1], ws[1], P[2] // ws[2], ws[2]).permute(0, 2, 4, 1, 3, 5)
    return lab.reshape(-1, ws[0] * ws[1] * ws[2])


def compute_mask_from_labels(labels: torch.Tensor) -> torch.Tensor:
    """(nW, n, n) additive mask: -100 where the labels of query and key differ, else 0 (MONAI's compute_mask)."""
    diff = labels[:, None, :] - labels[:, :, None]
    return torch.where(diff != 0, torch.tensor(-100.0), torch.tensor(0.0))


# ---------------------------------------------------------------------------------------------------- parameter holders
class PatchEmbed(nn.Module):
    def __init__(self, in_chans: int, embed_dim: int):
        super().__init__()
        self.patch_size = (PATCH,) * 3
        self.embed_dim = embed_dim
        self.proj = nn.Conv3d(in_chans, embed_dim, kernel_size=PATCH, stride=PATCH)


class WindowAttention(nn.Module):
    def __init__(self, dim: int, num_heads: int, qkv_bias: bool = True, attn_drop: float = 0.0, proj_drop: float = 0.0):
        super().__init__()
        self.dim, self.num_heads = dim, num_heads
        self.window_size = (WINDOW,) * 3
        self.scale = (dim // num_heads) ** -0.5
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * WINDOW - 1) ** 3, num_heads))
        self.register_buffer("relative_position_index", relative_position_index())
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        with torch.no_grad():
            nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)
        self.softmax = nn.Softmax(dim=-1)


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim: int, num_heads: int, shift: bool, drop: float, attn_drop: float, drop_path: float):
        super().__init__()
        self.dim, self.num_heads = dim, num_heads
        self.window_size = (WINDOW,) * 3
        self.shift_size = (WINDOW // 2,) * 3 if shift else (0, 0, 0)
        self.drop_path_rate = float(drop_path)
        self.norm1 = nn.LayerNorm(dim)
        self.attn = WindowAttention(dim, num_heads, True, attn_drop, drop)
        self.drop_path = nn.Identity()
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = MLPBlock(dim, int(dim * MLP_RATIO), drop)


class PatchMerging(nn.Module):
    """monai.networks.nets.swin_unetr.PatchMerging (v1, "merging"): cat of the 8 offsets in MONAI's legacy order -> norm -> reduction."""

    def __init__(self, dim: int):
        super().__init__()
        self.dim = dim
        self.reduction = nn.Linear(8 * dim, 2 * dim, bias=False)
        self.norm = nn.LayerNorm(8 * dim)


class BasicLayer(nn.Module):
    def __init__(self, dim: int, depth: int, num_heads: int, drop_path: Sequence[float], drop: float, attn_drop: float):
        super().__init__()
        self.window_size = (WINDOW,) * 3
        self.shift_size = (WINDOW // 2,) * 3
        self.no_shift = (0, 0, 0)
        self.depth = depth
        self.blocks = nn.ModuleList([SwinTransformerBlock(dim, num_heads, i % 2 == 1, drop, attn_drop, drop_path[i])
                                     for i in range(depth)])
        self.downsample = PatchMerging(dim)


class SwinTransformer(nn.Module):
    def __init__(self, in_chans: int, embed_dim: int, drop_rate: float, attn_drop_rate: float, drop_path_rate: float):
        super().__init__()
        self.num_layers = len(DEPTHS)
        self.embed_dim = embed_dim
        self.patch_embed = PatchEmbed(in_chans, embed_dim)
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, sum(DEPTHS))]
        for i in range(self.num_layers):
            layer = BasicLayer(int(embed_dim * 2 ** i), DEPTHS[i], NUM_HEADS[i], dpr[sum(DEPTHS[:i]):sum(DEPTHS[:i + 1])], drop_rate,
                               attn_drop_rate)
            setattr(self, f"layers{i + 1}", nn.ModuleList([layer]))


class SwinUNETR(nn.Module):
    """monai.networks.nets.SwinUNETR (MONAI 1.3, spatial_dims 3, v1 merging) with the same child names, so state-dict keys
    interchange."""

    def __init__(self, img_size: Sequence[int], in_channels: int, out_channels: int, feature_size: int = 24, norm_name="instance",
                 drop_rate: float = 0.0, attn_drop_rate: float = 0.0, dropout_path_rate: float = 0.0, normalize: bool = True,
                 use_checkpoint: bool = False):
        super().__init__()
        img_size = tuple(int(s) for s in img_size)
        if len(img_size) == 2:
            raise NotImplementedError("monai_swin_unetr: the MI355X engine builds the 3-D SwinUNETR only (input_size has 2 axes)")
        if len(img_size) != 3:
            raise ValueError(f"monai_swin_unetr: model.input_size must have 3 axes, got {list(img_size)}")
        for m in img_size:
            if m % STAGE_FACTOR != 0:
                raise ValueError("input image size (img_size) should be divisible by stage-wise image resolution.")
        if not 0 <= drop_rate <= 1:
            raise ValueError("dropout rate should be between 0 and 1.")
        if not 0 <= attn_drop_rate <= 1:
            raise ValueError("attention dropout rate should be between 0 and 1.")
        if not 0 <= dropout_path_rate <= 1:
            raise ValueError("drop path rate should be between 0 and 1.")
        if feature_size % 12 != 0:
            raise ValueError("feature_size should be divisible by 12.")
        if feature_size // 3 not in WINDOW_HEAD_DIMS:
            raise NotImplementedError(f"monai_swin_unetr: head width feature_size / 3 = {feature_size // 3} has no HIP window-attention "
                                      "kernel (16 or 32: feature_size 48 or 96)")
        _unetr_norm(norm_name, 1)        # refuse an unsupported norm before building anything
        self.img_size = img_size
        self.feature_size = fs = int(feature_size)
        self.normalize = bool(normalize)
        self.use_checkpoint = bool(use_checkpoint)
        self.drop_rate, self.attn_drop_rate, self.dropout_path_rate = float(drop_rate), float(attn_drop_rate), float(dropout_path_rate)
        self.swinViT = SwinTransformer(in_channels, fs, drop_rate, attn_drop_rate, dropout_path_rate)
        self.encoder1 = UnetrBasicBlock(in_channels, fs, norm_name)
        self.encoder2 = UnetrBasicBlock(fs, fs, norm_name)
        self.encoder3 = UnetrBasicBlock(2 * fs, 2 * fs, norm_name)
        self.encoder4 = UnetrBasicBlock(4 * fs, 4 * fs, norm_name)
        self.encoder10 = UnetrBasicBlock(16 * fs, 16 * fs, norm_name)
        self.decoder5 = UnetrUpBlock(16 * fs, 8 * fs, norm_name)
        self.decoder4 = UnetrUpBlock(8 * fs, 4 * fs, norm_name)
        self.decoder3 = UnetrUpBlock(4 * fs, 2 * fs, norm_name)
        self.decoder2 = UnetrUpBlock(2 * fs, fs, norm_name)
        self.decoder1 = UnetrUpBlock(fs, fs, norm_name)
        self.out = UnetOutBlock(fs, out_channels)

    def forward(self, x):  # pragma: no cover - guard only
        raise RuntimeError("the MONAI-style SwinUNETR executes through MONAIModelWrapper.forward (HIP engine); its modules are "
                           "parameter holders")


# ---------------------------------------------------------------------------------------------------- HIP execution
def _ln(norm, x: torch.Tensor) -> torch.Tensor:
    from ...training.swin_autograd import LayerNormRowsFn
    if norm is None:                                             # proj_out: F.layer_norm without affine
        return LayerNormRowsFn.apply(x, None, None, 1e-5)
    return LayerNormRowsFn.apply(x, norm.weight, norm.bias, norm.eps)


def _swin_block(blk: SwinTransformerBlock, x: torch.Tensor, B: int, grid, window, shift) -> torch.Tensor:
    """x + reverse(proj(attn(qkv(partition(norm1 x))))), then + linear2(GELU(linear1(norm2 x))); x a (B * D * H * W, dim) matrix."""
    from ... import hip_ops as ops
    from ...training.swin_autograd import WindowAttentionFn, WindowPartitionFn, WindowReverseFn
    from ...training.transformer_autograd import LinearFn
    a = blk.attn
    w = WindowPartitionFn.apply(_ln(blk.norm1, x), B, grid, window, shift)       # padding after norm1: pad rows are exact zeros
    n = window[0] * window[1] * window[2]
    qkv = LinearFn.apply(w, a.qkv.weight, a.qkv.bias, None, False)
    o = WindowAttentionFn.apply(qkv, a.relative_position_bias_table, int(w.shape[0]) // n, a.num_heads,
                                ops.window_attention_geom(grid, window, shift))
    x = WindowReverseFn.apply(LinearFn.apply(o, a.proj.weight, a.proj.bias, None, False), x, B, grid, window, shift)
    mp = blk.mlp
    a1 = LinearFn.apply(_ln(blk.norm2, x), mp.linear1.weight, mp.linear1.bias, None, False)
    return LinearFn.apply(a1, mp.linear2.weight, mp.linear2.bias, x, True)         # GELU applied to the pre-activation as it is read


def _merge(m: PatchMerging, x: torch.Tensor, B: int, grid):
    from ...training.swin_autograd import SpaceToDepth2Fn
    from ...training.transformer_autograd import LinearFn
    cols = SpaceToDepth2Fn.apply(x.view(B, *grid, int(x.shape[-1])), 1)
    return LinearFn.apply(_ln(m.norm, cols), m.reduction.weight, None, None, False), tuple(g // 2 for g in grid)


def check_input_size(spatial) -> None:
    wrong = [i for i, s in enumerate(spatial) if int(s) % STAGE_FACTOR != 0]
    if wrong:
        raise ValueError(f"spatial dimensions {wrong} of input image (spatial shape: {tuple(int(s) for s in spatial)}) must be divisible "
                         f"by {PATCH}**5.")


def swin_vit_forward(net: SwinUNETR, x: torch.Tensor) -> list:
    """The Swin encoder (MONAI's `swinViT(x, normalize)`) on channels-last x -> its five hidden states, channels-last
    (B, D / 2^(i+1), H / 2^(i+1), W / 2^(i+1), fs 2^i), each after proj_out when net.normalize."""
    from ...training.swin_autograd import PatchEmbed2Fn
    check_input_size(x.shape[1:4])
    if net.training and (net.drop_rate > 0 or net.attn_drop_rate > 0 or net.dropout_path_rate > 0):
        raise NotImplementedError(f"monai_swin_unetr: dropout {net.drop_rate}, attention dropout {net.attn_drop_rate} or drop path "
                                  f"{net.dropout_path_rate} > 0 in training mode has no HIP kernel (they must be 0.0)")
    B = int(x.shape[0])
    vit = net.swinViT
    pe = vit.patch_embed.proj
    grid = tuple(int(s) // PATCH for s in x.shape[1:4])
    t = PatchEmbed2Fn.apply(x, pe.weight, pe.bias)

    def out(z, g):
        z = _ln(None, z) if net.normalize else z
        return z.view(B, *g, int(z.shape[-1]))

    hidden = [out(t, grid)]
    for i in range(vit.num_layers):
        layer = getattr(vit, f"layers{i + 1}")[0]
        window, shift = get_window_size(grid, layer.window_size, layer.shift_size)
        for blk in layer.blocks:
            t = _swin_block(blk, t, B, grid, window, shift if any(blk.shift_size) else (0, 0, 0))
        t, grid = _merge(layer.downsample, t, B, grid)
        hidden.append(out(t, grid))
    return hidden


def swin_unetr_forward(net: SwinUNETR, x: torch.Tensor) -> torch.Tensor:
    """SwinUNETR on channels-last x (B, D, H, W, C_in) -> (B, D, H, W, C_out); nothing is built lazily or shared between calls (safe
    on the window engine's side streams).  Any spatial size whose axes divide by 32 runs: no embedding is tied to input_size."""
    hidden = swin_vit_forward(net, x)
    enc0 = _res_block(net.encoder1.layer, x)
    enc1 = _res_block(net.encoder2.layer, hidden[0])
    enc2 = _res_block(net.encoder3.layer, hidden[1])
    enc3 = _res_block(net.encoder4.layer, hidden[2])
    dec4 = _res_block(net.encoder10.layer, hidden[4])
    u = _up(net.decoder5, dec4, hidden[3])
    u = _up(net.decoder4, u, enc3)
    u = _up(net.decoder3, u, enc2)
    u = _up(net.decoder2, u, enc1)
    u = _up(net.decoder1, u, enc0)
    return _conv(net.out.conv, u)


@register_architecture("monai_swin_unetr")
def build_swin_unetr(cfg) -> ConnectomicsModel:
    """MONAI SwinUNETR: model.input_size, model.{in,out}_channels, model.transformer.{feature_size 48, dropout 0.0, attn_drop_rate 0.0,
    dropout_path_rate 0.0, use_checkpoint False} (reference monai_models.py:297-334); everything else MONAI's defaults -- in particular
    instance norm: transformer.norm is not passed, as in the reference."""
    tc = getattr(cfg.model, "transformer", None)
    size = getattr(cfg.model, "input_size", None)
    if not size:
        raise ValueError("monai_swin_unetr needs model.input_size (MONAI's img_size)")
    model = SwinUNETR(
        img_size=list(size), in_channels=cfg.model.in_channels, out_channels=cfg.model.out_channels,
        feature_size=getattr(tc, "feature_size", 48), use_checkpoint=getattr(tc, "use_checkpoint", False),
        drop_rate=getattr(tc, "dropout", 0.0), attn_drop_rate=getattr(tc, "attn_drop_rate", 0.0),
        dropout_path_rate=getattr(tc, "dropout_path_rate", 0.0))
    return MONAIModelWrapper(model)


__all__ = ["SwinUNETR", "SwinTransformer", "BasicLayer", "SwinTransformerBlock", "WindowAttention", "PatchMerging", "PatchEmbed",
           "get_window_size", "relative_position_index", "sliced_index", "kernel_index", "mask_region_labels",
           "compute_mask_from_labels", "check_input_size", "swin_vit_forward", "swin_unetr_forward", "build_swin_unetr"]

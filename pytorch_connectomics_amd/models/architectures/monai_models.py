"""MONAI-style residual U-Net on the MI355X -- counterpart of the `monai_unet` architecture of the reference
(connectomics/models/architectures/monai_models.py: MONAIModelWrapper :29-55, `_infer_spatial_dims` :66-70, `_resolve_norm`
:73-79, UpsampleModeUNet :84-139, build_monai_unet :197-250), which delegates the network itself to the third-party,
un-vendored `monai` package (`monai.networks.nets.UNet`, `monai.networks.blocks.{Convolution, ResidualUnit, ADN}`).

The module tree below restates that published architecture with the SAME child names, so state-dict keys interchange
(`model.model.0.conv.unit0.conv.weight`, `...adn.N.running_mean`, `...adn.A.weight`, `model.model.1.submodule...`,
`model.model.2.0.conv.weight` ...):

    UNet.model   = Sequential(down, SkipConnection(sub-block), up)            channel concat skip
    down         = ResidualUnit(in, c, stride 2, subunits = num_res_units)    conv k3 s2 -> ADN -> conv k3 -> ADN, + residual
                   residual = Conv3d(k3, s2, p1) when strided, Conv3d(k1) when only the width changes, Identity otherwise
    bottom       = ResidualUnit(c, c_last, stride 1)
    up           = Sequential(Convolution(transposed k3 s2 p1 op1 -> ADN), ResidualUnit(out, out, subunits 1,
                   last_conv_only = is_top))
    ADN ("NDA")  = norm (batch | instance | group) -> Dropout(p) -> PReLU (one weight, 0.25)

The torch.nn children are parameter holders.  `forward` runs hand-written gfx950 kernels on NDHWC tensors through the
autograd Functions of training/rsunet_autograd.py (dense conv3d on MFMA; the stride-2 / transposed resampling convs
in csrc/conv3d_strided_kernels.hip; norm statistics, affine + PReLU, their backward kernels), in training and inference.
No CPU path.

`monai_basic_unet3d` (build_basic_unet, reference monai_models.py:142-194) restates monai.networks.nets.BasicUNet the same way
(`model.conv_0.conv_0.conv.weight`, `model.down_1.convs.conv_1.adn.N.running_mean`, `model.upcat_4.upsample.deconv.weight`,
`model.final_conv.weight`): TwoConv / Down(MaxPool3d 2, TwoConv) / UpCat(deconv k2 s2 -> replicate pad to the skip -> cat([skip, up])
-> TwoConv), ADN = norm -> dropout -> relu | leakyrelu | prelu | elu.  Each UpCat's deconv, pad and concat are ONE fused kernel pair
(csrc/upcat_kernels.hip through training/rsunet_autograd.py UpCatFn).
"""
from __future__ import annotations

from typing import Optional, Sequence, Union

import torch
import torch.nn as nn

from .base import ConnectomicsModel
from .mednext import resolve_compute_dtype, to_channels_first, to_channels_last
from .registry import register_architecture

MONAI_AVAILABLE = True      # the architecture is built in-repo; nothing to import


def _same_padding(kernel_size: int) -> int:
    if (kernel_size - 1) % 2 == 1:
        raise NotImplementedError(f"Same padding not available for kernel_size={kernel_size}.")
    return (kernel_size - 1) // 2


def _make_norm(norm, channels: int) -> nn.Module:
    """MONAI norm factory for the three spellings `_resolve_norm` can hand over (monai_models.py:73-79)."""
    args = {}
    if isinstance(norm, (tuple, list)):
        norm, args = norm[0], dict(norm[1])
    name = str(norm).lower()
    if name == "batch":
        return nn.BatchNorm3d(channels, **args)
    if name == "instance":
        return nn.InstanceNorm3d(channels, **args)
    if name == "group":
        return nn.GroupNorm(num_channels=channels, **args)
    raise ValueError(f"Unsupported MONAI norm {norm!r} for the MI355X engine (batch, instance, group)")


_ACTS = {"relu": nn.ReLU, "leakyrelu": nn.LeakyReLU, "prelu": nn.PReLU, "elu": nn.ELU}


def _make_act(act) -> nn.Module:
    """MONAI activation factory for the four activations the norm + activation kernels implement: a name, or (name, kwargs) as MONAI
    spells it; defaults are torch's (LeakyReLU slope 0.01, PReLU one weight 0.25, ELU alpha 1)."""
    args = {}
    if isinstance(act, (tuple, list)):
        act, args = act[0], {k: v for k, v in dict(act[1]).items() if k != "inplace"}
    name = str(act).lower()
    if name not in _ACTS:
        raise NotImplementedError(f"MONAI activation {act!r} has no HIP kernel (supported: {', '.join(_ACTS)})")
    return _ACTS[name](**args)


class ADN(nn.Sequential):
    """norm -> dropout -> activation ("NDA"), children named N / D / A as in monai.networks.blocks.ADN."""

    def __init__(self, channels: int, norm, dropout: Optional[float], act="prelu"):
        super().__init__()
        self.add_module("N", _make_norm(norm, channels))
        if dropout is not None:
            self.add_module("D", nn.Dropout(float(dropout)))
        self.add_module("A", _make_act(act))


class Convolution(nn.Sequential):
    """conv (or transposed conv) [+ ADN] -- monai.networks.blocks.Convolution for spatial_dims = 3."""

    def __init__(self, in_channels: int, out_channels: int, strides: int = 1, kernel_size: int = 3, norm="instance",
                 dropout: Optional[float] = None, bias: bool = True, conv_only: bool = False, is_transposed: bool = False,
                 act="prelu"):
        super().__init__()
        pad = _same_padding(kernel_size)
        if is_transposed:
            conv = nn.ConvTranspose3d(in_channels, out_channels, kernel_size, stride=strides, padding=pad,
                                      output_padding=strides - 1, bias=bias)
        else:
            conv = nn.Conv3d(in_channels, out_channels, kernel_size, stride=strides, padding=pad, bias=bias)
        self.add_module("conv", conv)
        if not conv_only:
            self.add_module("adn", ADN(out_channels, norm, dropout, act))


class ResidualUnit(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, strides: int = 1, kernel_size: int = 3, subunits: int = 2,
                 norm="instance", dropout: Optional[float] = None, bias: bool = True, last_conv_only: bool = False):
        super().__init__()
        self.conv = nn.Sequential()
        self.residual: nn.Module = nn.Identity()
        pad = _same_padding(kernel_size)
        sch, sst = in_channels, strides
        subunits = max(1, subunits)
        for su in range(subunits):
            conv_only = last_conv_only and su == subunits - 1
            self.conv.add_module(f"unit{su:d}", Convolution(sch, out_channels, strides=sst, kernel_size=kernel_size,
                                                            norm=norm, dropout=dropout, bias=bias, conv_only=conv_only))
            sch, sst = out_channels, 1
        if strides != 1 or in_channels != out_channels:
            rk, rp = kernel_size, pad
            if strides == 1:            # only the width changes: 1x1x1, no padding
                rk, rp = 1, 0
            self.residual = nn.Conv3d(in_channels, out_channels, rk, strides, rp, bias=bias)


class SkipConnection(nn.Module):
    """cat([x, submodule(x)], channel dim) -- monai.networks.layers.SkipConnection(mode='cat')."""

    def __init__(self, submodule: nn.Module):
        super().__init__()
        self.submodule = submodule


class UNet(nn.Module):
    """monai.networks.nets.UNet (spatial_dims = 3, act = PReLU, adn_ordering = 'NDA', up_kernel_size = 3)."""

    def __init__(self, spatial_dims: int, in_channels: int, out_channels: int, channels: Sequence[int],
                 strides: Sequence[int], kernel_size: int = 3, up_kernel_size: int = 3, num_res_units: int = 0,
                 norm="instance", dropout: float = 0.0, bias: bool = True):
        super().__init__()
        if spatial_dims != 3:
            raise NotImplementedError("the MI355X engine builds the 3-D MONAI U-Net only (spatial_dims=3)")
        if len(channels) < 2:
            raise ValueError("the length of `channels` should be no less than 2.")
        delta = len(strides) - (len(channels) - 1)
        if delta < 0:
            raise ValueError("the length of `strides` should equal to `len(channels) - 1`.")
        self.dimensions = spatial_dims
        self.in_channels, self.out_channels = in_channels, out_channels
        self.channels, self.strides = tuple(channels), tuple(strides)
        self.kernel_size, self.up_kernel_size = kernel_size, up_kernel_size
        self.num_res_units, self.norm, self.dropout, self.bias = num_res_units, norm, dropout, bias

        def create(inc: int, outc: int, chans: Sequence[int], strs: Sequence[int], is_top: bool) -> nn.Module:
            c, s = chans[0], strs[0]
            if len(chans) > 2:
                sub = create(c, c, chans[1:], strs[1:], False)
                upc = c * 2
            else:
                sub = self._down(c, chans[1], 1)                       # bottom layer
                upc = c + chans[1]
            return nn.Sequential(self._down(inc, c, s), SkipConnection(sub), self._up(upc, outc, s, is_top))

        self.model = create(in_channels, out_channels, self.channels, self.strides, True)

    def _down(self, inc: int, outc: int, strides: int) -> nn.Module:
        """monai UNet._get_down_layer: a ResidualUnit, or with num_res_units = 0 one plain Convolution (conv -> norm -> PReLU)."""
        if self.num_res_units > 0:
            return ResidualUnit(inc, outc, strides=strides, kernel_size=self.kernel_size, subunits=self.num_res_units,
                                norm=self.norm, dropout=self.dropout, bias=self.bias)
        return Convolution(inc, outc, strides=strides, kernel_size=self.kernel_size, norm=self.norm, dropout=self.dropout,
                           bias=self.bias)

    def _up(self, inc: int, outc: int, strides: int, is_top: bool) -> nn.Module:
        """monai UNet._get_up_layer: transposed Convolution (+ a one-subunit ResidualUnit when num_res_units > 0); the top layer ends
        without norm / activation -- on the ResidualUnit's last conv, or with num_res_units = 0 on the transposed conv itself."""
        conv = Convolution(inc, outc, strides=strides, kernel_size=self.up_kernel_size, norm=self.norm,
                           dropout=self.dropout, bias=self.bias, conv_only=is_top and self.num_res_units == 0, is_transposed=True)
        if self.num_res_units <= 0:
            return conv
        ru = ResidualUnit(outc, outc, strides=1, kernel_size=self.kernel_size, subunits=1, norm=self.norm,
                          dropout=self.dropout, bias=self.bias, last_conv_only=is_top)
        return nn.Sequential(conv, ru)

    def forward(self, x):  # pragma: no cover - guard only
        raise RuntimeError("the MONAI-style UNet executes through MONAIModelWrapper.forward (HIP engine); its modules are "
                           "parameter holders")


class UpsampleModeUNet(UNet):
    """Name kept from the reference (monai_models.py:84-139); only the default transposed-conv upsampling is built."""

    def __init__(self, upsample_mode: str = "deconv", upsample_interp_mode: str = "linear",
                 upsample_align_corners: bool = True, **kwargs):
        if upsample_mode and upsample_mode != "deconv":
            raise NotImplementedError(f"monai_unet upsample_mode={upsample_mode!r}: only 'deconv' has HIP kernels")
        self.upsample_mode = upsample_mode
        self.upsample_interp_mode = upsample_interp_mode
        self.upsample_align_corners = upsample_align_corners
        super().__init__(**kwargs)


# ---------------------------------------------------------------------------------------------------- HIP execution
def _adn(adn: ADN, x: torch.Tensor) -> torch.Tensor:
    from ...training.rsunet_autograd import NormActFn
    n = adn.N
    drop = getattr(adn, "D", None)
    if drop is not None and drop.p > 0 and drop.training:
        raise NotImplementedError("dropout > 0 in training mode has no HIP kernel (monai.dropout must be 0.0)")
    if isinstance(n, nn.BatchNorm3d):
        kind, groups, bn = "batch", 1, n
    elif isinstance(n, nn.GroupNorm):
        kind, groups, bn = "group", n.num_groups, None
    else:
        kind, groups, bn = "instance", 1, None
    a = adn.A
    if isinstance(a, nn.PReLU):
        act_kind, prm, prelu_w = "prelu", 0.0, a.weight
    elif isinstance(a, nn.LeakyReLU):
        act_kind, prm, prelu_w = "leakyrelu", float(a.negative_slope), None
    elif isinstance(a, nn.ELU):
        act_kind, prm, prelu_w = "elu", float(a.alpha), None
    else:
        act_kind, prm, prelu_w = "relu", 0.0, None
    return NormActFn.apply(x, getattr(n, "weight", None), getattr(n, "bias", None), prelu_w, kind, groups,
                           float(n.eps), act_kind, prm, bn)


def _convolution(m: Convolution, x: torch.Tensor) -> torch.Tensor:
    from ...training.rsunet_autograd import ResampleConv3dFn
    y = ResampleConv3dFn.apply(x, m.conv.weight, m.conv.bias, int(m.conv.stride[0]), int(m.conv.padding[0]),
                               isinstance(m.conv, nn.ConvTranspose3d))
    return _adn(m.adn, y) if hasattr(m, "adn") else y


def _residual_unit(m: ResidualUnit, x: torch.Tensor) -> torch.Tensor:
    from ...training.rsunet_autograd import AddFn, ResampleConv3dFn
    if isinstance(m.residual, nn.Identity):
        res = x
    else:
        r = m.residual
        res = ResampleConv3dFn.apply(x, r.weight, r.bias, int(r.stride[0]), int(r.padding[0]), False)
    cx = x
    for unit in m.conv:
        cx = _convolution(unit, cx)
    return AddFn.apply(cx, res)


def _run(mod: nn.Module, x: torch.Tensor) -> torch.Tensor:
    if isinstance(mod, ResidualUnit):
        return _residual_unit(mod, x)
    if isinstance(mod, Convolution):
        return _convolution(mod, x)
    if isinstance(mod, SkipConnection):
        y = _run(mod.submodule, x)
        if tuple(y.shape[1:4]) != tuple(x.shape[1:4]):
            # what torch.cat raises inside MONAI's SkipConnection, spelled out
            raise ValueError(f"monai_unet skip connection: spatial size {tuple(x.shape[1:4])} is not restored by the "
                             f"down/up path (got {tuple(y.shape[1:4])}); every spatial size must be divisible by "
                             "the product of the strides")
        return torch.cat([x, y], dim=-1)
    if isinstance(mod, nn.Sequential):
        for child in mod:
            x = _run(child, x)
        return x
    raise TypeError(f"unexpected module in the MONAI U-Net tree: {type(mod).__name__}")


# ------------------------------------------------------------------------------------------------------ MONAI BasicUNet
class TwoConv(nn.Sequential):
    """monai.networks.nets.basic_unet.TwoConv: two Convolution(k3, p1) -> ADN ("NDA") units."""

    def __init__(self, in_chns: int, out_chns: int, act, norm, bias: bool, dropout: float = 0.0):
        super().__init__()
        self.add_module("conv_0", Convolution(in_chns, out_chns, norm=norm, dropout=dropout, bias=bias, act=act))
        self.add_module("conv_1", Convolution(out_chns, out_chns, norm=norm, dropout=dropout, bias=bias, act=act))


class Down(nn.Sequential):
    """monai.networks.nets.basic_unet.Down: MaxPool3d(2) -> TwoConv."""

    def __init__(self, in_chns: int, out_chns: int, act, norm, bias: bool, dropout: float = 0.0):
        super().__init__()
        self.add_module("max_pooling", nn.MaxPool3d(kernel_size=2))
        self.add_module("convs", TwoConv(in_chns, out_chns, act, norm, bias, dropout))


class UpSample(nn.Sequential):
    """monai.networks.blocks.UpSample(mode="deconv", scale_factor=2): one ConvTranspose3d(k 2, stride 2) named `deconv`."""

    def __init__(self, in_channels: int, out_channels: int, bias: bool = True):
        super().__init__()
        self.add_module("deconv", nn.ConvTranspose3d(in_channels, out_channels, kernel_size=2, stride=2, bias=bias))


class UpCat(nn.Module):
    """monai.networks.nets.basic_unet.UpCat: up-sample, replicate-pad to the skip's size, cat([skip, up]), TwoConv."""

    def __init__(self, in_chns: int, cat_chns: int, out_chns: int, act, norm, bias: bool, dropout: float = 0.0,
                 upsample: str = "deconv", halves: bool = True):
        super().__init__()
        if upsample != "deconv":
            raise NotImplementedError(f"monai_basic_unet3d upsample_mode={upsample!r}: only 'deconv' has HIP kernels "
                                      "('nontrainable' and 'pixelshuffle' are not built)")
        up_chns = in_chns // 2 if halves else in_chns
        self.upsample = UpSample(in_chns, up_chns, bias)
        self.convs = TwoConv(cat_chns + up_chns, out_chns, act, norm, bias, dropout)


class BasicUNet(nn.Module):
    """monai.networks.nets.BasicUNet (spatial_dims = 3) with the same child names, so state-dict keys interchange."""

    def __init__(self, spatial_dims: int = 3, in_channels: int = 1, out_channels: int = 2,
                 features: Sequence[int] = (32, 32, 64, 128, 256, 32), act="relu", norm="batch", bias: bool = True,
                 dropout: float = 0.0, upsample: str = "deconv"):
        super().__init__()
        if spatial_dims != 3:
            raise NotImplementedError("the MI355X engine builds the 3-D MONAI BasicUNet only (spatial_dims=3)")
        if upsample != "deconv":
            raise NotImplementedError(f"monai_basic_unet3d upsample_mode={upsample!r}: only 'deconv' has HIP kernels "
                                      "('nontrainable' and 'pixelshuffle' are not built)")
        fea = tuple(int(f) for f in features)
        if len(fea) != 6:
            raise ValueError(f"BasicUNet needs 6 feature sizes, got {len(fea)}")
        self.features = fea
        self.conv_0 = TwoConv(in_channels, fea[0], act, norm, bias, dropout)
        self.down_1 = Down(fea[0], fea[1], act, norm, bias, dropout)
        self.down_2 = Down(fea[1], fea[2], act, norm, bias, dropout)
        self.down_3 = Down(fea[2], fea[3], act, norm, bias, dropout)
        self.down_4 = Down(fea[3], fea[4], act, norm, bias, dropout)
        self.upcat_4 = UpCat(fea[4], fea[3], fea[3], act, norm, bias, dropout, upsample)
        self.upcat_3 = UpCat(fea[3], fea[2], fea[2], act, norm, bias, dropout, upsample)
        self.upcat_2 = UpCat(fea[2], fea[1], fea[1], act, norm, bias, dropout, upsample)
        self.upcat_1 = UpCat(fea[1], fea[0], fea[5], act, norm, bias, dropout, upsample, halves=False)
        self.final_conv = nn.Conv3d(fea[5], out_channels, kernel_size=1)

    def forward(self, x):  # pragma: no cover - guard only
        raise RuntimeError("the MONAI-style BasicUNet executes through MONAIModelWrapper.forward (HIP engine); its modules are "
                           "parameter holders")


def _two_conv(m: TwoConv, x: torch.Tensor) -> torch.Tensor:
    return _convolution(m.conv_1, _convolution(m.conv_0, x))


def _up_cat(m: UpCat, x_low: torch.Tensor, x_e: torch.Tensor) -> torch.Tensor:
    from ...training.rsunet_autograd import UpCatFn
    d = m.upsample.deconv
    return _two_conv(m.convs, UpCatFn.apply(x_e, x_low, d.weight, d.bias))


def basic_unet_forward(net: BasicUNet, x: torch.Tensor) -> torch.Tensor:
    """BasicUNet on channels-last x (N, D, H, W, C): TwoConv / MaxPool / fused UpCat / 1x1 conv, every piece a HIP kernel with its own
    autograd backward; nothing is built lazily or shared between calls (safe on the window engine's side streams)."""
    from ...training.rsunet_autograd import MaxPoolFn, ResampleConv3dFn
    for axis, size in zip("DHW", x.shape[1:4]):
        if int(size) < 16:
            raise ValueError(f"monai_basic_unet3d: spatial axis {axis} has {int(size)} voxels; four 2x max-poolings need at least 16")
    x0 = _two_conv(net.conv_0, x)
    x1 = _two_conv(net.down_1.convs, MaxPoolFn.apply(x0, (2, 2, 2)))
    x2 = _two_conv(net.down_2.convs, MaxPoolFn.apply(x1, (2, 2, 2)))
    x3 = _two_conv(net.down_3.convs, MaxPoolFn.apply(x2, (2, 2, 2)))
    x4 = _two_conv(net.down_4.convs, MaxPoolFn.apply(x3, (2, 2, 2)))
    u = _up_cat(net.upcat_4, x4, x3)
    u = _up_cat(net.upcat_3, u, x2)
    u = _up_cat(net.upcat_2, u, x1)
    u = _up_cat(net.upcat_1, u, x0)
    f = net.final_conv
    return ResampleConv3dFn.apply(u, f.weight, f.bias, 1, 0, False)


class MONAIModelWrapper(ConnectomicsModel):
    """ConnectomicsModel interface over the MONAI-style network; single-scale output (no deep supervision)."""

    def __init__(self, model: nn.Module):
        super().__init__()
        self.model = model
        self.supports_deep_supervision = False
        self.output_scales = 1
        self.compute_dtype: Optional[torch.dtype] = None       # None -> follow autocast

    def forward_cl(self, x_cl: torch.Tensor) -> torch.Tensor:
        """Channels-last entry of the sliding-window engine: (N,D,H,W,C_in) -> (N,D,H,W,C_out) fp32."""
        if not x_cl.is_cuda:
            raise RuntimeError(f"{self._arch} (pytorch_connectomics_amd) runs only on an MI355X/ROCm device: "
                               "there is no CPU path. Move the model and input to 'cuda'.")
        from ...training.rsunet_autograd import prefetch_prelu, refresh_conv_packs
        prefetch_prelu([m.weight for m in self.model.modules() if isinstance(m, nn.PReLU)])   # one host read, not one per layer
        refresh_conv_packs()          # every conv-weight image whose weight changed since the last forward, in one launch
        dt = resolve_compute_dtype(self.compute_dtype)
        x = x_cl if x_cl.dtype == dt else x_cl.to(dt)
        if isinstance(self.model, BasicUNet):
            return basic_unet_forward(self.model, x.contiguous()).float()
        from .unetr import UNETR, unetr_forward
        if isinstance(self.model, UNETR):
            return unetr_forward(self.model, x.contiguous()).float()
        from .swin_unetr import SwinUNETR, swin_unetr_forward
        if isinstance(self.model, SwinUNETR):
            return swin_unetr_forward(self.model, x.contiguous()).float()
        return _run(self.model.model, x.contiguous()).float()

    @property
    def _arch(self) -> str:
        from .swin_unetr import SwinUNETR
        from .unetr import UNETR
        if isinstance(self.model, UNETR):
            return "monai_unetr"
        if isinstance(self.model, SwinUNETR):
            return "monai_swin_unetr"
        return "monai_basic_unet3d" if isinstance(self.model, BasicUNet) else "monai_unet"

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda:
            raise RuntimeError(f"{self._arch} (pytorch_connectomics_amd) runs only on an MI355X/ROCm device: "
                               "there is no CPU path. Move the model and input to 'cuda'.")
        if x.dim() != 5:
            name = {"monai_basic_unet3d": "BasicUNet", "monai_unetr": "UNETR",
                    "monai_swin_unetr": "SwinUNETR"}.get(self._arch, "U-Net")
            raise NotImplementedError(f"the MI355X engine runs the 3-D MONAI {name} on (B, C, D, H, W) inputs")
        y = self.forward_cl(to_channels_last(x.float()))
        return y.permute(0, 4, 1, 2, 3) if y.requires_grad else to_channels_first(y)


def _infer_spatial_dims(cfg) -> int:
    if hasattr(cfg.model, "input_size") and cfg.model.input_size:
        return len(cfg.model.input_size)
    return getattr(cfg.model.monai, "spatial_dims", 3)


def _resolve_norm(cfg):
    norm_type = getattr(cfg.model.monai, "norm", "batch")
    if norm_type == "group":
        return ("group", {"num_groups": getattr(cfg.model.monai, "num_groups", 8)})
    return norm_type


def _basic_unet_features(filters) -> tuple:
    """BasicUNet takes exactly six feature sizes: pad with the last value repeated, then truncate (monai_models.py:178-182)."""
    fea = [int(f) for f in filters]
    if not fea:
        raise ValueError("model.monai.filters must not be empty")
    while len(fea) < 6:
        fea.append(fea[-1])
    return tuple(fea[:6])


@register_architecture("monai_basic_unet3d")
def build_basic_unet(cfg) -> ConnectomicsModel:
    """MONAI BasicUNet: model.monai.{filters (padded / truncated to 6), dropout, activation, norm, num_groups, upsample_mode};
    (monai_models.py:142-194).  Only upsample_mode='deconv' is built."""
    mc = cfg.model.monai
    model = BasicUNet(
        spatial_dims=_infer_spatial_dims(cfg), in_channels=cfg.model.in_channels, out_channels=cfg.model.out_channels,
        features=_basic_unet_features(getattr(mc, "filters", [32, 64, 128, 256, 512])),
        dropout=getattr(mc, "dropout", 0.0), act=getattr(mc, "activation", "relu"), norm=_resolve_norm(cfg),
        upsample=getattr(mc, "upsample_mode", "deconv"))
    return MONAIModelWrapper(model)


@register_architecture("monai_unet")
def build_monai_unet(cfg) -> ConnectomicsModel:
    """MONAI UNet with residual units: model.monai.{filters, num_res_units, kernel_size, norm, num_groups, dropout,
    upsample_mode}; 2x down-sampling at every level (strides = [2] * (len(filters) - 1), monai_models.py:228-229)."""
    mc = cfg.model.monai
    channels = list(getattr(mc, "filters", [32, 64, 128, 256, 512]))
    model = UpsampleModeUNet(
        spatial_dims=_infer_spatial_dims(cfg), in_channels=cfg.model.in_channels, out_channels=cfg.model.out_channels,
        channels=channels, strides=[2] * (len(channels) - 1), num_res_units=getattr(mc, "num_res_units", 2),
        kernel_size=getattr(mc, "kernel_size", 3), norm=_resolve_norm(cfg), dropout=getattr(mc, "dropout", 0.0),
        upsample_mode=getattr(mc, "upsample_mode", "deconv"),
        upsample_interp_mode=getattr(mc, "upsample_interp_mode", "linear"),
        upsample_align_corners=getattr(mc, "upsample_align_corners", True))
    return MONAIModelWrapper(model)


__all__ = ["MONAIModelWrapper", "UpsampleModeUNet", "UNet", "ResidualUnit", "Convolution", "ADN", "SkipConnection",
           "BasicUNet", "TwoConv", "Down", "UpSample", "UpCat", "basic_unet_forward", "build_basic_unet", "build_monai_unet"]

"""GPU checks of `monai_swin_unetr` (MONAI SwinUNETR): the window-attention, window partition / reverse, space-to-depth and LayerNorm
kernels against float64 torch, the whole network against a functional torch restatement of MONAI 1.3 that reads the HIP model's own
state_dict, one training step against float64 autograd, bit-reproducibility, the absence of torch glue ops, the device-side refusals,
the sliding-window engine and the CLI."""
import copy
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_connectomics_amd.models.architectures.swin_unetr import (compute_mask_from_labels, get_window_size, mask_region_labels,
                                                                    relative_position_index)

pytestmark = pytest.mark.gpu


def _relmax(a, r):
    a, r = a.detach().double(), r.detach().double()
    return float((a - r).abs().max() / r.abs().max().clamp_min(1e-30))


def _cl(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _padded(grid, ws):
    return [-(-g // w) * w for g, w in zip(grid, ws)]


# ----------------------------------------------------------------------------------------------------- window attention
def _win_attn_ref(qkv, table, nwin, heads, ws, shift, padded):
    n = ws[0] * ws[1] * ws[2]
    hid = qkv.shape[1] // 3
    d = hid // heads
    q, k, v = qkv.reshape(nwin, n, 3, heads, d).permute(2, 0, 3, 1, 4)
    att = (q * d ** -0.5) @ k.transpose(-1, -2)
    bias = table[relative_position_index()[:n, :n].reshape(-1)].reshape(n, n, heads).permute(2, 0, 1)
    att = att + bias.unsqueeze(0)
    if any(shift):
        mask = compute_mask_from_labels(mask_region_labels(padded, ws, shift)).to(att.dtype)
        nw = mask.shape[0]
        att = (att.view(nwin // nw, nw, heads, n, n) + mask.unsqueeze(1).unsqueeze(0)).view(nwin, heads, n, n)
    return (torch.softmax(att, -1) @ v).permute(0, 2, 1, 3).reshape(nwin * n, hid)


_WIN_CASES = [((7, 7, 7), (9, 7, 12)), ((6, 6, 6), (6, 12, 6)), ((4, 7, 7), (4, 8, 8)), ((2, 2, 2), (2, 4, 2))]


@pytest.mark.parametrize("ws,grid", _WIN_CASES)
@pytest.mark.parametrize("d", [16, 32])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dt,tol", [(torch.float32, 1e-4), (torch.bfloat16, 3e-2)])
def test_window_attention_matches_float64(ws, grid, d, masked, dt, tol):
    from pytorch_connectomics_amd import hip_ops as ops
    from pytorch_connectomics_amd.training.swin_autograd import WindowAttentionFn
    heads, B = 3, 2
    shift = tuple(min(3, w - 1) if (masked and w > 1) else 0 for w in ws)
    if masked and ws == (4, 7, 7):
        shift = (0, 3, 3)                                  # what get_window_size gives on a (4, 8, 8) stage
    padded = _padded(grid, ws)
    n = ws[0] * ws[1] * ws[2]
    nwin = B * (padded[0] // ws[0]) * (padded[1] // ws[1]) * (padded[2] // ws[2])
    g = torch.Generator().manual_seed(n + d + masked)
    qkv = (torch.randn(nwin * n, 3 * heads * d, generator=g) * 1.5).to(dt).float()
    table = 0.5 * torch.randn(2197, heads, generator=g)
    dout = torch.randn(nwin * n, heads * d, generator=g).to(dt).float()
    q_ref, t_ref = qkv.double().requires_grad_(True), table.double().requires_grad_(True)
    o_ref = _win_attn_ref(q_ref, t_ref, nwin, heads, ws, shift, padded)
    o_ref.backward(dout.double())
    geom = ops.window_attention_geom(grid, ws, shift)
    qg, tg = qkv.to(dt).cuda().requires_grad_(True), table.cuda().requires_grad_(True)
    o = WindowAttentionFn.apply(qg, tg, nwin, heads, geom)
    o.backward(dout.to(dt).cuda())
    assert o.dtype == dt and o.shape == (nwin * n, heads * d)
    assert _relmax(o.float().cpu(), o_ref) <= tol
    hid = heads * d
    for part, sl in (("dQ", slice(0, hid)), ("dK", slice(hid, 2 * hid)), ("dV", slice(2 * hid, 3 * hid))):
        assert _relmax(qg.grad[:, sl].float().cpu(), q_ref.grad[:, sl]) <= tol, part
    assert _relmax(tg.grad.cpu(), t_ref.grad) <= tol, "relative_position_bias_table"
    # rows of the table no query / key pair reads get exactly zero
    used = torch.zeros(2197, dtype=torch.bool)
    used[relative_position_index()[:n, :n].reshape(-1)] = True
    assert torch.equal(tg.grad.cpu()[~used], torch.zeros_like(tg.grad.cpu()[~used]))
    # the backward twice: bit-identical (no atomics)
    first_q, first_t = qg.grad.clone(), tg.grad.clone()
    qg.grad = tg.grad = None
    WindowAttentionFn.apply(qg, tg, nwin, heads, geom).backward(dout.to(dt).cuda())
    assert torch.equal(first_q, qg.grad) and torch.equal(first_t, tg.grad)


def test_window_attention_head_widths():
    from pytorch_connectomics_amd import hip_ops as ops
    assert ops.window_attention_supported(16) and ops.window_attention_supported(32)
    assert not ops.window_attention_supported(64) and not ops.window_attention_supported(24)


# ------------------------------------------------------------------------------------------- partition / reverse
def _partition_ref(x, B, grid, ws, shift):
    C = x.shape[-1]
    v = x.view(B, *grid, C)
    pad = [p - g for p, g in zip(_padded(grid, ws), grid)]
    v = F.pad(v, (0, 0, 0, pad[2], 0, pad[1], 0, pad[0]))
    if any(shift):
        v = torch.roll(v, shifts=tuple(-s for s in shift), dims=(1, 2, 3))
    P = v.shape[1:4]
    v = v.view(B, P[0] // ws[0], ws[0], P[1] // ws[1], ws[1], P[2] // ws[2], ws[2], C).permute(0, 1, 3, 5, 2, 4, 6, 7)
    return v.reshape(-1, C)


@pytest.mark.parametrize("grid,ws,shift", [((9, 7, 12), (7, 7, 7), (3, 0, 3)), ((4, 8, 8), (4, 7, 7), (0, 3, 3)),
                                           ((16, 16, 16), (7, 7, 7), (3, 3, 3)), ((6, 10, 3), (6, 7, 3), (0, 3, 0)),
                                           ((5, 6, 7), (5, 6, 7), (0, 0, 0))])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_window_partition_and_reverse_match_torch(grid, ws, shift, dt):
    from pytorch_connectomics_amd.training.swin_autograd import WindowPartitionFn, WindowReverseFn
    B, C = 2, 48
    g = torch.Generator().manual_seed(sum(grid) + sum(shift))
    x = torch.randn(B * grid[0] * grid[1] * grid[2], C, generator=g).to(dt)
    ref = _partition_ref(x, B, grid, ws, shift)
    xg = x.cuda().requires_grad_(True)
    w = WindowPartitionFn.apply(xg, B, grid, ws, shift)
    assert torch.equal(w.cpu(), ref)
    dw = torch.randn(w.shape, generator=g).to(dt)
    w.backward(dw.cuda())
    xr = x.double().requires_grad_(True)
    _partition_ref(xr, B, grid, ws, shift).backward(dw.double())
    assert torch.equal(xg.grad.cpu().double(), xr.grad)
    # reverse with the residual: crop(roll back(windows)) + res, and its gradient
    res = torch.randn(x.shape, generator=g).to(dt)
    wg, rg = dw.cuda().requires_grad_(True), res.cuda().requires_grad_(True)
    y = WindowReverseFn.apply(wg, rg, B, grid, ws, shift)
    wr = dw.double().requires_grad_(True)
    xr2 = torch.zeros(x.shape, dtype=torch.float64, requires_grad=True)
    # the reverse is the adjoint of the partition restricted to real tokens: find it by the partition's autograd
    inv = torch.autograd.grad(_partition_ref(xr2, B, grid, ws, shift), xr2, wr, create_graph=True)[0]
    yr = inv + res.double()
    tol = 1e-6 if dt == torch.float32 else 1e-2
    assert float((y.cpu().double() - yr).abs().max()) <= tol * float(yr.abs().max())
    dy = torch.randn(y.shape, generator=g).to(dt)
    y.backward(dy.cuda())
    assert torch.equal(rg.grad.cpu(), dy)
    assert torch.equal(wg.grad.cpu(), _partition_ref(dy, B, grid, ws, shift))


# ---------------------------------------------------------------------------------------------------- space-to-depth
_V1 = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 0), (0, 0, 1), (1, 1, 1)]


def _s2d_ref(x, order):
    offs = [(s >> 2, (s >> 1) & 1, s & 1) for s in range(8)] if order == 0 else _V1
    return torch.cat([x[:, a::2, b::2, c::2, :] for a, b, c in offs], -1).reshape(-1, 8 * x.shape[-1])


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("C", [1, 2, 48, 96])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_space_to_depth_matches_torch(order, C, dt):
    from pytorch_connectomics_amd.training.swin_autograd import SpaceToDepth2Fn
    g = torch.Generator().manual_seed(C + 7 * order)
    x = torch.randn(2, 4, 6, 8, C, generator=g).to(dt)
    xg = x.cuda().requires_grad_(True)
    y = SpaceToDepth2Fn.apply(xg, order)
    assert torch.equal(y.cpu(), _s2d_ref(x, order))
    dy = torch.randn(y.shape, generator=g).to(dt)
    y.backward(dy.cuda())
    xr = x.double().requires_grad_(True)
    _s2d_ref(xr, order).backward(dy.double())
    assert _relmax(xg.grad.cpu(), xr.grad) <= (1e-6 if dt == torch.float32 else 1e-2)
    if order == 1:       # offsets (1,1,0) and (0,1,1) are never read: exactly zero gradient
        assert torch.equal(xg.grad[:, 1::2, 1::2, 0::2].cpu(), torch.zeros_like(xg.grad[:, 1::2, 1::2, 0::2].cpu()))
        assert torch.equal(xg.grad[:, 0::2, 1::2, 1::2].cpu(), torch.zeros_like(xg.grad[:, 0::2, 1::2, 1::2].cpu()))


def test_patch_embedding_matches_conv3d():
    from pytorch_connectomics_amd.training.swin_autograd import PatchEmbed2Fn
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 2, 8, 6, 4, generator=g)
    w = 0.3 * torch.randn(48, 2, 2, 2, 2, generator=g)
    b = 0.1 * torch.randn(48, generator=g)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    yr = F.conv3d(xr, wr, br, stride=2)
    dy = torch.randn(yr.shape, generator=g)
    yr.backward(dy.double())
    xg, wg, bg = _cl(x).cuda().requires_grad_(True), w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = PatchEmbed2Fn.apply(xg, wg, bg)
    y.backward(_cl(dy).reshape(-1, 48).cuda())
    assert _relmax(y.cpu(), _cl(yr.detach()).reshape(-1, 48)) <= 1e-5
    assert _relmax(xg.grad.cpu(), _cl(xr.grad)) <= 1e-5
    assert _relmax(wg.grad.cpu(), wr.grad) <= 1e-5 and _relmax(bg.grad.cpu(), br.grad) <= 1e-5


# ------------------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("C", [48, 96, 1536, 3072, 6144])
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("dt,tol", [(torch.float32, 1e-4), (torch.bfloat16, 3e-2)])
def test_layernorm_rows_matches_torch(C, affine, dt, tol):
    from pytorch_connectomics_amd.training.swin_autograd import LayerNormRowsFn
    g = torch.Generator().manual_seed(C + affine)
    rows = 437 if C <= 1536 else 75
    x = (torch.randn(rows, C, generator=g) * 2 + 0.5).to(dt).float()
    w = 1 + 0.3 * torch.randn(C, generator=g)
    b = 0.2 * torch.randn(C, generator=g)
    dy = torch.randn(rows, C, generator=g).to(dt).float()
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    yr = F.layer_norm(xr, (C,), wr if affine else None, br if affine else None, 1e-5)
    yr.backward(dy.double())
    xg = x.to(dt).cuda().requires_grad_(True)
    wg, bg = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = LayerNormRowsFn.apply(xg, wg if affine else None, bg if affine else None, 1e-5)
    y.backward(dy.to(dt).cuda())
    assert _relmax(y.float().cpu(), yr.detach()) <= tol
    assert _relmax(xg.grad.float().cpu(), xr.grad) <= tol
    if affine:
        assert _relmax(wg.grad.cpu(), wr.grad) <= tol and _relmax(bg.grad.cpu(), br.grad) <= tol


# ------------------------------------------------------------------------------------------------------- whole network
def _cfg(size=(64, 64, 64), fs=48, c_in=1, c_out=2, **extra):
    return NS(model=NS(arch=NS(type="monai_swin_unetr"), in_channels=c_in, out_channels=c_out, input_size=list(size),
                       transformer=NS(feature_size=fs, **extra)))


def _model(cfg, seed=0):
    """The HIP model in a 'trained' state: non-trivial LayerNorm affine, biases and bias tables."""
    from pytorch_connectomics_amd.models import build_model
    torch.manual_seed(seed)
    m = build_model(cfg)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if ".norm" in n or n.endswith(".bias"):
                p.add_(0.1 * torch.randn(p.shape, generator=g))
            if "relative_position_bias_table" in n:
                p.mul_(10.0)
            if n.endswith("conv.weight") and "transp" not in n:
                p.mul_(2.0)
    return m


class RefSwinUNETR:
    """Functional torch restatement of MONAI 1.3 SwinUNETR (v1 merging, instance norm) over a state dict with the wrapper's keys."""

    def __init__(self, m, dtype=torch.float32):
        self.p = {k[len("model."):]: (v.detach().clone().to(dtype) if v.is_floating_point() else v.detach().clone())
                  for k, v in m.state_dict().items()}
        for v in self.p.values():
            if v.is_floating_point():
                v.requires_grad_(True)
        self.used = set()

    def __getitem__(self, k):
        self.used.add(k)
        return self.p[k]

    def _res(self, x, pre):
        y = F.conv3d(x, self[pre + ".conv1.conv.weight"], padding=1)
        y = F.leaky_relu(F.instance_norm(y, eps=1e-5), 0.01)
        y = F.instance_norm(F.conv3d(y, self[pre + ".conv2.conv.weight"], padding=1), eps=1e-5)
        r = x
        if pre + ".conv3.conv.weight" in self.p:
            r = F.instance_norm(F.conv3d(x, self[pre + ".conv3.conv.weight"]), eps=1e-5)
        return F.leaky_relu(y + r, 0.01)

    def _lin(self, x, pre, bias=True):
        return F.linear(x, self[pre + ".weight"], self[pre + ".bias"] if bias else None)

    def _ln(self, x, pre):
        return F.layer_norm(x, (x.shape[-1],), self[pre + ".weight"], self[pre + ".bias"], 1e-5)

    def _attn(self, x, pre, heads, mask):
        b_, n, c = x.shape
        qkv = self._lin(x, pre + ".qkv").reshape(b_, n, 3, heads, c // heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        q = q * (c // heads) ** -0.5
        attn = q @ k.transpose(-2, -1)
        idx = self[pre + ".relative_position_index"].clone()[:n, :n].reshape(-1)
        bias = self[pre + ".relative_position_bias_table"][idx].reshape(n, n, -1).permute(2, 0, 1).contiguous()
        attn = attn + bias.unsqueeze(0)
        if mask is not None:
            nw = mask.shape[0]
            attn = attn.view(b_ // nw, nw, heads, n, n) + mask.to(attn.dtype).unsqueeze(1).unsqueeze(0)
            attn = attn.view(-1, heads, n, n)
        attn = torch.softmax(attn, -1).to(v.dtype)
        x = (attn @ v).transpose(1, 2).reshape(b_, n, c)
        return self._lin(x, pre + ".proj")

    def _block(self, x, pre, heads, shifted):
        b, d, h, w, c = x.shape
        ws, ss = get_window_size((d, h, w), (7, 7, 7), (3, 3, 3))
        if not shifted:
            ss = (0, 0, 0)
        shortcut = x
        x = self._ln(x, pre + ".norm1")
        pad = [(ws[i] - s % ws[i]) % ws[i] for i, s in enumerate((d, h, w))]
        x = F.pad(x, (0, 0, 0, pad[2], 0, pad[1], 0, pad[0]))
        _, dp, hp, wp, _ = x.shape
        mask = None
        if any(s > 0 for s in ss):
            x = torch.roll(x, shifts=(-ss[0], -ss[1], -ss[2]), dims=(1, 2, 3))
            mask = compute_mask_from_labels(mask_region_labels((dp, hp, wp), ws, ss))
        xw = x.view(b, dp // ws[0], ws[0], hp // ws[1], ws[1], wp // ws[2], ws[2], c).permute(0, 1, 3, 5, 2, 4, 6, 7)
        xw = xw.reshape(-1, ws[0] * ws[1] * ws[2], c)
        aw = self._attn(xw, pre + ".attn", heads, mask)
        x = aw.view(b, dp // ws[0], hp // ws[1], wp // ws[2], ws[0], ws[1], ws[2], c).permute(0, 1, 4, 2, 5, 3, 6, 7)
        x = x.reshape(b, dp, hp, wp, c)
        if any(s > 0 for s in ss):
            x = torch.roll(x, shifts=ss, dims=(1, 2, 3))
        x = shortcut + x[:, :d, :h, :w].contiguous()
        y = F.gelu(self._lin(self._ln(x, pre + ".norm2"), pre + ".mlp.linear1"))
        return x + self._lin(y, pre + ".mlp.linear2")

    def _merge(self, x, pre):
        xs = [x[:, a::2, b::2, c::2, :] for a, b, c in _V1]
        return self._lin(self._ln(torch.cat(xs, -1), pre + ".norm"), pre + ".reduction", bias=False)

    def encoder(self, x):
        """swinViT(x, normalize=True): the five hidden states, channels-last."""
        t = F.conv3d(x, self["swinViT.patch_embed.proj.weight"], self["swinViT.patch_embed.proj.bias"], stride=2)
        t = t.permute(0, 2, 3, 4, 1)
        hs = [F.layer_norm(t, [t.shape[-1]])]
        for i in range(4):
            pre = f"swinViT.layers{i + 1}.0"
            for b in range(2):
                t = self._block(t, f"{pre}.blocks.{b}", 3 * 2 ** i, b == 1)
            t = self._merge(t, pre + ".downsample")
            hs.append(F.layer_norm(t, [t.shape[-1]]))
        return hs

    def __call__(self, x):
        hs = [h.permute(0, 4, 1, 2, 3) for h in self.encoder(x)]

        def up(z, skip, pre):
            z = F.conv_transpose3d(z, self[pre + ".transp_conv.conv.weight"], stride=2)
            return self._res(torch.cat([z, skip], 1), pre + ".conv_block")

        enc0 = self._res(x, "encoder1.layer")
        enc1 = self._res(hs[0], "encoder2.layer")
        enc2 = self._res(hs[1], "encoder3.layer")
        enc3 = self._res(hs[2], "encoder4.layer")
        dec4 = self._res(hs[4], "encoder10.layer")
        u = up(dec4, hs[3], "decoder5")
        u = up(u, enc3, "decoder4")
        u = up(u, enc2, "decoder3")
        u = up(u, enc1, "decoder2")
        u = up(u, enc0, "decoder1")
        return F.conv3d(u, self["out.conv.conv.weight"], self["out.conv.conv.bias"])


@pytest.mark.parametrize("size,fs,B", [((64, 64, 64), 48, 1), ((32, 64, 96), 48, 2), ((64, 64, 64), 96, 1)])
def test_swin_unetr_forward_matches_torch(size, fs, B):
    m = _model(_cfg(size, fs, c_in=1, c_out=2))
    ref_net = RefSwinUNETR(m)
    x = torch.rand(B, 1, *size, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        ref = ref_net(x)
        assert ref_net.used == set(ref_net.p)                           # every key, the index buffers included
        m = m.cuda().eval()
        got = m(x.cuda()).cpu()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            got16 = m(x.cuda()).float().cpu()
        with torch.autocast("cpu", dtype=torch.bfloat16):
            ref16 = ref_net(x).float()
    assert got.shape == ref.shape == (B, 2) + tuple(size) and got.dtype == torch.float32
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    print("fp32 max error", err, "range", scale)
    assert err <= 1e-3 * scale
    err16, ref_err16 = float((got16 - ref).abs().max()), float((ref16 - ref).abs().max())
    print("bf16 max error", err16, "CPU autocast", ref_err16)
    assert err16 <= 1.5 * ref_err16, (err16, ref_err16)


def _loss(y, tgt):
    p = torch.sigmoid(y)
    dice = 1 - (2 * (p * tgt).sum() + 1e-5) / (p.sum() + tgt.sum() + 1e-5)
    return F.binary_cross_entropy_with_logits(y, tgt) + dice


def test_swin_encoder_gradients_match_float64():
    """The Swin encoder alone (every kernel of this architecture but the shared decoder blocks), 32 x 64 x 64 with stage grids
    16x32x32, 8x16x16, 4x8x8 (window (4, 7, 7), shift (0, 3, 3)) and 2x4x4: loss = sum_i <w_i, hidden_i>.  Measured worst per-tensor
    relative L2 error 4e-6."""
    from pytorch_connectomics_amd.models.architectures.swin_unetr import swin_vit_forward
    m = _model(_cfg((32, 64, 64), 48, c_out=1), seed=4)
    ref_net = RefSwinUNETR(m, torch.float64)
    x = torch.rand(1, 1, 32, 64, 64, generator=torch.Generator().manual_seed(5))
    hs = ref_net.encoder(x.double())
    g = torch.Generator().manual_seed(9)
    ws = [torch.randn(h.shape, generator=g) for h in hs]
    sum((h * w.double()).sum() for h, w in zip(hs, ws)).backward()
    m = m.cuda().train()
    got = swin_vit_forward(m.model, _cl(x).cuda())
    assert [tuple(h.shape) for h in got] == [tuple(h.shape) for h in hs]
    for h, r in zip(got, hs):
        assert _relmax(h.cpu(), r) <= 1e-4
    sum((h * w.cuda()).sum() for h, w in zip(got, ws)).backward()
    worst = (0.0, "")
    for k, p in m.named_parameters():
        if ".swinViT." not in k:
            continue
        r = ref_net.p[k[len("model."):]].grad
        worst = max(worst, (float((p.grad.cpu().double() - r).norm() / r.norm().clamp_min(1e-30)), k))
    print("worst encoder gradient error", worst)
    assert worst[0] <= 1e-4, worst


def test_swin_unetr_training_step_matches_torch_autograd():
    """32 x 64 x 64: stage grids 16x32x32, 8x16x16, 4x8x8 (window (4, 7, 7), shift (0, 3, 3)), 2x4x4.  The encoder's own error is
    4e-6 (test above); through the decoder, the stage-2 gradients of this configuration are ill-conditioned (torch's own fp32 step
    is off by 3e-3 there) and the shared instance-norm statistics of the UNETR decoder blocks bring ours to 7.6e-3,
    2.4x torch's floor: the bound is 3x that floor where it exceeds 2e-3/3."""
    m = _model(_cfg((32, 64, 64), 48, c_out=1), seed=4)
    st0 = copy.deepcopy(m.state_dict())
    ref_net = RefSwinUNETR(m, torch.float64)
    x = torch.rand(1, 1, 32, 64, 64, generator=torch.Generator().manual_seed(5))
    tgt = (torch.rand(1, 1, 32, 64, 64, generator=torch.Generator().manual_seed(6)) > 0.7).float()
    ref_loss = _loss(ref_net(x.double()), tgt.double())
    ref_loss.backward()
    ref32 = RefSwinUNETR(m)
    _loss(ref32(x), tgt).backward()
    m = m.cuda().train()
    loss = _loss(m(x.cuda()), tgt.cuda())
    loss.backward()
    assert abs(float(loss.detach()) - float(ref_loss.detach())) <= 1e-4 * max(1.0, abs(float(ref_loss)))
    worst = (0.0, "", 0.0, 0.0)
    names = set()
    for k, p in m.named_parameters():
        names.add(k)
        r = ref_net.p[k[len("model."):]].grad
        assert p.grad is not None and r is not None, k
        rel = float((p.grad.cpu().double() - r.double()).norm() / r.double().norm().clamp_min(1e-30))
        floor = float((ref32.p[k[len("model."):]].grad.double() - r.double()).norm() / r.double().norm().clamp_min(1e-30))
        worst = max(worst, (rel / max(2e-3, 3.0 * floor), k, rel, floor))
    print("worst gradient error / bound", worst)
    assert worst[0] <= 1.0, worst
    assert any("relative_position_bias_table" in k for k in names) and any("downsample.reduction" in k for k in names)

    def step():
        m.load_state_dict(st0)
        opt = torch.optim.SGD(m.parameters(), lr=0.1)
        opt.zero_grad(set_to_none=True)
        _loss(m(x.cuda()), tgt.cuda()).backward()
        opt.step()
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in m.state_dict().items()}
    a, b = step(), step()
    for k in a:
        assert torch.equal(a[k], b[k]), k


_GLUE = ("aten::bmm", "aten::matmul", "aten::mm", "aten::addmm", "aten::linear", "aten::softmax", "aten::_softmax", "aten::layer_norm",
         "aten::native_layer_norm", "aten::gelu", "aten::cat", "aten::scaled_dot_product_attention", "aten::roll",
         "aten::constant_pad_nd", "aten::pad", "aten::index", "aten::index_select", "aten::gather", "aten::index_add",
         "aten::scatter_add")


def test_swin_unetr_runs_no_torch_glue():
    m = _model(_cfg((32, 64, 64), 48, c_out=1), seed=2).cuda().train()
    x = torch.rand(1, 1, 32, 64, 64, device="cuda")
    tgt = (torch.rand(1, 1, 32, 64, 64, device="cuda") > 0.5).float()
    F.binary_cross_entropy_with_logits(m(x), tgt).backward()          # warm-up: weight images, library load
    torch.cuda.synchronize()
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        F.binary_cross_entropy_with_logits(m(x), tgt).backward()
        torch.cuda.synchronize()
    names = {e.key for e in prof.key_averages()}
    bad = sorted(n for n in names if n in _GLUE or n.startswith("aten::conv") or n.startswith("aten::_conv")
                 or n.startswith("aten::miopen") or n.startswith("aten::_scaled_dot") or n.startswith("aten::_flash"))
    assert not bad, bad


def test_swin_unetr_refusals_on_the_device():
    m = _model(_cfg((32, 32, 32), 48)).cuda()
    with pytest.raises(ValueError, match="divisible"):
        with torch.no_grad():
            m.eval()(torch.rand(1, 1, 48, 48, 48).cuda())
    for key in ("dropout", "attn_drop_rate", "dropout_path_rate"):
        md = _model(_cfg((32, 32, 32), 48, **{key: 0.1})).cuda()
        with torch.no_grad():
            assert torch.isfinite(md.eval()(torch.rand(1, 1, 32, 32, 32).cuda())).all()     # eval: the identity
        with pytest.raises(NotImplementedError, match="training mode"):
            md.train()(torch.rand(1, 1, 32, 32, 32).cuda())


def test_swin_unetr_in_sliding_window_engine():
    """Built with input_size 64^3, run with 32 x 64 x 64 windows (no embedding is tied to input_size)."""
    from pytorch_connectomics_amd.inference.window import EagerSlidingWindowEngine
    m = _model(_cfg((64, 64, 64), 48, c_out=1), seed=9).cuda().eval()
    one = torch.rand(1, 1, 32, 64, 64, generator=torch.Generator().manual_seed(4)).cuda()
    eng1 = EagerSlidingWindowEngine(roi_size=(32, 64, 64), sw_batch_size=1, overlap=0.5, mode="constant", padding_mode="constant",
                                    cval=0.0)
    with torch.no_grad():
        got = eng1(one, m)
        direct = m(one)
    torch.testing.assert_close(got, direct, rtol=1e-6, atol=1e-6)
    vol = torch.rand(1, 1, 48, 80, 72, generator=torch.Generator().manual_seed(2)).cuda()
    eng = EagerSlidingWindowEngine(roi_size=(32, 64, 64), sw_batch_size=2, overlap=0.5, mode="bump", padding_mode="constant",
                                   cval=0.0)
    with torch.no_grad():
        out = eng(vol, m)
    assert out.shape == (1, 1, 48, 80, 72) and torch.isfinite(out).all()


def test_cli_swin_unetr_train_then_test(tmp_path):
    """tutorials/minimal_swin_unetr.yaml as committed (only its output directory moved under tmp_path): trains two steps, then
    predicts."""
    import re
    from pathlib import Path
    from pytorch_connectomics_amd.inference.artifact import read_prediction_artifact
    from pytorch_connectomics_amd.main import main
    text = (Path(__file__).resolve().parents[1] / "tutorials" / "minimal_swin_unetr.yaml").read_text()
    cfg = tmp_path / "minimal_swin_unetr.yaml"
    cfg.write_text(re.sub(r"(?m)^save_path: .*$", f"save_path: {tmp_path / 'out'}", text, count=1))
    out = main(["--config", str(cfg), "--mode", "train"])
    assert out["steps"] == 2 and np.isfinite(out["first_loss"])
    ck = tmp_path / "out" / "checkpoints" / "last.ckpt"
    blob = torch.load(ck, weights_only=True)
    assert blob["global_step"] == 2
    assert "model.model.swinViT.layers4.0.blocks.1.attn.relative_position_bias_table" in blob["state_dict"]
    assert "model.model.decoder1.conv_block.conv3.conv.weight" in blob["state_dict"]
    res = main(["--config", str(cfg), "--mode", "test", "--checkpoint", str(ck)])
    assert res["output_voxels_per_s"] > 0
    pred = read_prediction_artifact(next((tmp_path / "out" / "results").glob("*_prediction.h5")))
    assert pred.shape == (1, 80, 96, 112) and np.isfinite(pred).all() and pred.std() > 0

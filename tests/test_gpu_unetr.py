"""GPU checks of `monai_unetr` (MONAI UNETR): the attention, wide LayerNorm, patch-embedding and k2/s2 deconv kernels against torch CPU
math, the whole network against a functional torch restatement that reads the HIP model's own state_dict, one training step against
torch autograd, bit-reproducibility, the absence of torch glue ops, the sliding-window engine and the CLI."""
import copy
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _relmax(a, r):
    a, r = a.detach().double(), r.detach().double()
    return float((a - r).abs().max() / r.abs().max().clamp_min(1e-30))


def _cl(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


# ------------------------------------------------------------------------------------------------------------ attention
def _attn_ref(qkv, B, heads):
    N = qkv.shape[0] // B
    hid = qkv.shape[1] // 3
    d = hid // heads
    q, k, v = qkv.double().reshape(B, N, 3, heads, d).permute(2, 0, 3, 1, 4)
    att = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, dim=-1)
    return (att @ v).permute(0, 2, 1, 3).reshape(B * N, hid)


@pytest.mark.parametrize("N,d,heads,B", [(8, 64, 1, 1), (27, 32, 3, 2), (216, 64, 12, 2), (512, 64, 2, 1), (512, 32, 4, 3),
                                         (216, 32, 5, 1)])
@pytest.mark.parametrize("dt,tol", [(torch.float32, 1e-4), (torch.bfloat16, 3e-2)])
def test_attention_matches_cpu_softmax(N, d, heads, B, dt, tol):
    from pytorch_connectomics_amd.training.transformer_autograd import AttentionFn
    g = torch.Generator().manual_seed(N * 7 + d + heads)
    qkv = (torch.randn(B * N, 3 * heads * d, generator=g) * 1.5).to(dt).float()
    dout = torch.randn(B * N, heads * d, generator=g).to(dt).float()
    q_ref = qkv.double().requires_grad_(True)
    o_ref = _attn_ref(q_ref, B, heads)
    o_ref.backward(dout.double())
    qg = qkv.to(dt).cuda().requires_grad_(True)
    o = AttentionFn.apply(qg, B, heads)
    o.backward(dout.to(dt).cuda())
    assert o.dtype == dt and o.shape == (B * N, heads * d)
    assert _relmax(o.float().cpu(), o_ref.detach()) <= tol
    hid = heads * d
    for part, sl in (("dQ", slice(0, hid)), ("dK", slice(hid, 2 * hid)), ("dV", slice(2 * hid, 3 * hid))):
        assert _relmax(qg.grad[:, sl].float().cpu(), q_ref.grad[:, sl]) <= tol, part
    # the backward twice: bit-identical (no atomics)
    first = qg.grad.clone()
    qg.grad = None
    AttentionFn.apply(qg, B, heads).backward(dout.to(dt).cuda())
    assert torch.equal(first, qg.grad)


# ------------------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("C", [192, 384, 768, 1024])
@pytest.mark.parametrize("dt,tol", [(torch.float32, 1e-4), (torch.bfloat16, 3e-2)])
def test_layernorm_wide_matches_torch(C, dt, tol):
    from pytorch_connectomics_amd.training.transformer_autograd import LayerNormFn
    g = torch.Generator().manual_seed(C)
    x = (torch.randn(437, C, generator=g) * 2 + 0.5).to(dt).float()
    w = 1 + 0.3 * torch.randn(C, generator=g)
    b = 0.2 * torch.randn(C, generator=g)
    dy = torch.randn(437, C, generator=g).to(dt).float()
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    yr = F.layer_norm(xr, (C,), wr, br, 1e-5)
    yr.backward(dy.double())
    xg = x.to(dt).cuda().requires_grad_(True)
    wg, bg = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = LayerNormFn.apply(xg, wg, bg, 1e-5)
    y.backward(dy.to(dt).cuda())
    assert _relmax(y.float().cpu(), yr.detach()) <= tol
    assert _relmax(xg.grad.float().cpu(), xr.grad) <= tol
    assert _relmax(wg.grad.cpu(), wr.grad) <= tol
    assert _relmax(bg.grad.cpu(), br.grad) <= tol


# ------------------------------------------------------------------------------------------------------ patch embedding
def _patches_ref(x, C):
    B, _, D, H, W = x.shape
    return (x.reshape(B, C, D // 16, 16, H // 16, 16, W // 16, 16).permute(0, 2, 4, 6, 3, 5, 7, 1)
            .reshape(B, (D // 16) * (H // 16) * (W // 16), 4096 * C))


@pytest.mark.parametrize("conv", [False, True])
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("dt,tol", [(torch.float32, 1e-4), (torch.bfloat16, 3e-2)])
def test_patch_embedding_matches_torch(conv, C, dt, tol):
    from pytorch_connectomics_amd.training.transformer_autograd import PatchEmbedFn
    g = torch.Generator().manual_seed(C + 10 * conv)
    B, hid, shape = 2, 192, (32, 48, 16)
    n = (32 // 16) * (48 // 16) * (16 // 16)
    x = torch.randn(B, C, *shape, generator=g).to(dt).float()
    w = 0.02 * torch.randn((hid, C, 16, 16, 16) if conv else (hid, 4096 * C), generator=g)
    b = 0.1 * torch.randn(hid, generator=g)
    pos = 0.1 * torch.randn(1, n, hid, generator=g)
    dy = torch.randn(B * n, hid, generator=g).to(dt).float()
    xr, wr, br, pr = (t.double().requires_grad_(True) for t in (x, w, b, pos))
    if conv:
        yr = F.conv3d(xr, wr, br, stride=16).flatten(2).transpose(1, 2) + pr
    else:
        yr = _patches_ref(xr, C) @ wr.t() + br + pr
    yr.reshape(B * n, hid).backward(dy.double())
    xg = _cl(x).to(dt).cuda().requires_grad_(True)
    wg, bg, pg = (t.cuda().requires_grad_(True) for t in (w, b, pos))
    y = PatchEmbedFn.apply(xg, wg, bg, pg, conv)
    y.backward(dy.to(dt).cuda())
    assert _relmax(y.float().cpu(), yr.detach().reshape(B * n, hid)) <= tol
    assert _relmax(xg.grad.float().cpu(), _cl(xr.grad)) <= tol
    for got, ref, name in ((wg.grad, wr.grad, "weight"), (bg.grad, br.grad, "bias"), (pg.grad, pr.grad, "position_embeddings")):
        assert got.shape == ref.shape, name
        assert _relmax(got.cpu(), ref) <= tol, name


# ------------------------------------------------------------------------------------------------- deconv k2 s2 (two forms)
@pytest.mark.parametrize("c_in,c_u,c_e", [(192, 16, 0), (16, 16, 0), (64, 32, 32), (16, 8, 8), (3, 5, 7)])
@pytest.mark.parametrize("dt,tol", [(torch.float32, 1e-4), (torch.bfloat16, 3e-2)])
def test_deconv2_upfirst_matches_deconv_cat(c_in, c_u, c_e, dt, tol):
    from pytorch_connectomics_amd.training.transformer_autograd import Deconv2Fn
    g = torch.Generator().manual_seed(c_in + c_u + c_e)
    low = (2, 3, 4, 5)
    x = torch.randn(low[0], c_in, *low[1:], generator=g).to(dt).float()
    w = 0.2 * torch.randn(c_in, c_u, 2, 2, 2, generator=g)
    skip = torch.randn(low[0], c_e, *(2 * s for s in low[1:]), generator=g).to(dt).float() if c_e else None
    dy = torch.randn(low[0], c_u + c_e, *(2 * s for s in low[1:]), generator=g).to(dt).float()
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    sr = skip.double().requires_grad_(True) if c_e else None
    yr = F.conv_transpose3d(xr, wr, stride=2)
    if c_e:
        yr = torch.cat([yr, sr], 1)
    yr.backward(dy.double())
    xg, wg = _cl(x).to(dt).cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    sg = _cl(skip).to(dt).cuda().requires_grad_(True) if c_e else None
    y = Deconv2Fn.apply(xg, wg, sg)
    y.backward(_cl(dy).to(dt).cuda())
    assert _relmax(y.float().cpu(), _cl(yr.detach())) <= tol
    assert _relmax(xg.grad.float().cpu(), _cl(xr.grad)) <= tol
    assert _relmax(wg.grad.cpu(), wr.grad) <= tol
    if c_e:
        assert torch.equal(sg.grad.float().cpu(), _cl(dy)[..., c_u:])


# ------------------------------------------------------------------------------------------------------------ linear layers
@pytest.mark.parametrize("K,N", [(768, 2304), (3072, 768), (192, 576), (96, 64)])
@pytest.mark.parametrize("x_gelu", [False, True])
@pytest.mark.parametrize("dt,tol", [(torch.float32, 1e-4), (torch.bfloat16, 3e-2)])
def test_linear_matches_torch(K, N, x_gelu, dt, tol):
    """y = f(x) W^T + b + res with f = GELU or identity; (768, 2304) / (3072, 768) in bf16 run on the pointwise MFMA GEMM, the rest on
    pytc_linear_*."""
    from pytorch_connectomics_amd import hip_ops as ops
    from pytorch_connectomics_amd.training.transformer_autograd import LinearFn
    g = torch.Generator().manual_seed(K + N + x_gelu)
    M = 437
    x = torch.randn(M, K, generator=g).to(dt).float()
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = 0.1 * torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g).to(dt).float()
    dy = torch.randn(M, N, generator=g).to(dt).float()
    xr, wr, br, rr = (t.double().requires_grad_(True) for t in (x, w, b, res))
    yr = (F.gelu(xr) if x_gelu else xr) @ wr.t() + br + rr
    yr.backward(dy.double())
    xg, rg = x.to(dt).cuda().requires_grad_(True), res.to(dt).cuda().requires_grad_(True)
    wg, bg = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = LinearFn.apply(xg, wg, bg, rg, x_gelu)
    y.backward(dy.to(dt).cuda())
    assert ops.linear_mfma_applies(xg, K, N) == (dt == torch.bfloat16 and K % 64 == 0 and N % 128 == 0)
    assert _relmax(y.float().cpu(), yr.detach()) <= tol
    for got, ref, name in ((xg.grad, xr.grad, "x"), (wg.grad, wr.grad, "weight"), (bg.grad, br.grad, "bias"), (rg.grad, rr.grad, "res")):
        assert _relmax(got.float().cpu(), ref) <= tol, name
    first = wg.grad.clone()
    wg.grad = None
    LinearFn.apply(xg, wg, bg, rg, x_gelu).backward(dy.to(dt).cuda())
    assert torch.equal(first, wg.grad)


# ------------------------------------------------------------------------------------------------------- whole network
def _cfg(size=(32, 32, 32), hid=192, heads=3, fs=8, mlp=256, norm="instance", pos="perceptron", c_in=1, c_out=2, dropout=0.0):
    return NS(model=NS(arch=NS(type="monai_unetr"), in_channels=c_in, out_channels=c_out, input_size=list(size),
                       transformer=NS(feature_size=fs, hidden_size=hid, mlp_dim=mlp, num_heads=heads, pos_embed=pos, norm=norm,
                                      dropout=dropout)))


def _model(cfg, seed=0):
    """The HIP model in a 'trained' state: non-trivial LayerNorm / BatchNorm affine and running statistics."""
    from pytorch_connectomics_amd.models import build_model
    torch.manual_seed(seed)
    m = build_model(cfg)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if ".norm" in n or "position_embeddings" in n or n.endswith(".bias"):
                p.add_(0.1 * torch.randn(p.shape, generator=g))
            if n.endswith("conv.weight") and "transp" not in n and "blocks" not in n:
                p.mul_(2.0)
        for n, b in m.named_buffers():
            if n.endswith("running_mean"):
                b.copy_(0.2 * torch.randn(b.shape, generator=g))
            if n.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
    return m


class RefUNETR:
    """Functional torch restatement of MONAI 1.3 UNETR over a state dict with the wrapper's keys (`model.` + MONAI key)."""

    def __init__(self, m, cfg, dtype=torch.float32):
        self.p = {k[len("model."):]: (v.detach().clone().to(dtype) if v.is_floating_point() else v.detach().clone())
                  for k, v in m.state_dict().items()}
        for k, v in self.p.items():
            if v.is_floating_point() and "running" not in k:
                v.requires_grad_(True)
        tc = cfg.model.transformer
        self.heads, self.hid, self.norm, self.pos = tc.num_heads, tc.hidden_size, tc.norm, tc.pos_embed
        self.size = tuple(cfg.model.input_size)
        self.used = set()

    def __getitem__(self, k):
        self.used.add(k)
        return self.p[k]

    def _norm(self, x, pre, training):
        if self.norm == "instance":
            return F.instance_norm(x, eps=1e-5)
        return F.batch_norm(x, self[pre + ".running_mean"].clone(), self[pre + ".running_var"].clone(), self[pre + ".weight"],
                            self[pre + ".bias"], training, 0.1, 1e-5)

    def _res(self, x, pre, training):
        y = F.conv3d(x, self[pre + ".conv1.conv.weight"], padding=1)
        y = F.leaky_relu(self._norm(y, pre + ".norm1", training), 0.01)
        y = self._norm(F.conv3d(y, self[pre + ".conv2.conv.weight"], padding=1), pre + ".norm2", training)
        r = x
        if pre + ".conv3.conv.weight" in self.p:
            r = self._norm(F.conv3d(x, self[pre + ".conv3.conv.weight"]), pre + ".norm3", training)
        return F.leaky_relu(y + r, 0.01)

    def _ln(self, t, pre):
        return F.layer_norm(t, (self.hid,), self[pre + ".weight"], self[pre + ".bias"], 1e-5)

    def __call__(self, x, training=False):
        B, C = x.shape[:2]
        fd = [s // 16 for s in self.size]
        pe = "vit.patch_embedding."
        if self.pos == "conv":
            t = F.conv3d(x, self[pe + "patch_embeddings.weight"], self[pe + "patch_embeddings.bias"], stride=16).flatten(2).transpose(1, 2)
        else:
            t = _patches_ref(x, C) @ self[pe + "patch_embeddings.1.weight"].t() + self[pe + "patch_embeddings.1.bias"]
        t = t + self[pe + "position_embeddings"]
        hs = []
        d = self.hid // self.heads
        for i in range(12):
            bp = f"vit.blocks.{i}."
            qkv = self._ln(t, bp + "norm1") @ self[bp + "attn.qkv.weight"].t()
            q, k, v = qkv.reshape(B, -1, 3, self.heads, d).permute(2, 0, 3, 1, 4)
            att = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, dim=-1)
            o = (att @ v).permute(0, 2, 1, 3).reshape(B, -1, self.hid)
            t = t + o @ self[bp + "attn.out_proj.weight"].t() + self[bp + "attn.out_proj.bias"]
            h = F.gelu(self._ln(t, bp + "norm2") @ self[bp + "mlp.linear1.weight"].t() + self[bp + "mlp.linear1.bias"])
            t = t + h @ self[bp + "mlp.linear2.weight"].t() + self[bp + "mlp.linear2.bias"]
            hs.append(t)
        t = self._ln(t, "vit.norm")

        def proj(z):
            return z.reshape(B, *fd, self.hid).permute(0, 4, 1, 2, 3)

        def pr_up(z, pre, n):
            z = F.conv_transpose3d(z, self[pre + ".transp_conv_init.conv.weight"], stride=2)
            for j in range(n):
                z = F.conv_transpose3d(z, self[f"{pre}.blocks.{j}.0.conv.weight"], stride=2)
                z = self._res(z, f"{pre}.blocks.{j}.1", training)
            return z

        def up(z, skip, pre):
            z = F.conv_transpose3d(z, self[pre + ".transp_conv.conv.weight"], stride=2)
            return self._res(torch.cat([z, skip], 1), pre + ".conv_block", training)

        enc1 = self._res(x, "encoder1.layer", training)
        enc2 = pr_up(proj(hs[3]), "encoder2", 2)
        enc3 = pr_up(proj(hs[6]), "encoder3", 1)
        enc4 = pr_up(proj(hs[9]), "encoder4", 0)
        u = up(proj(t), enc4, "decoder5")
        u = up(u, enc3, "decoder4")
        u = up(u, enc2, "decoder3")
        u = up(u, enc1, "decoder2")
        return F.conv3d(u, self["out.conv.conv.weight"], self["out.conv.conv.bias"])


@pytest.mark.parametrize("size,hid,heads,fs,norm,pos", [
    ((32, 32, 32), 192, 3, 8, "instance", "perceptron"),
    ((32, 32, 32), 192, 3, 8, "batch", "conv"),
    ((64, 64, 64), 384, 6, 16, "instance", "conv"),
    ((64, 64, 64), 384, 6, 16, "batch", "perceptron"),
])
def test_unetr_forward_matches_torch(size, hid, heads, fs, norm, pos):
    cfg = _cfg(size, hid, heads, fs, 2 * hid, norm, pos)
    m = _model(cfg)
    ref_net = RefUNETR(m, cfg)
    x = torch.rand(2, 1, *size, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        ref = ref_net(x)
        assert ref_net.used == set(k for k in ref_net.p if "num_batches" not in k)
        m = m.cuda().eval()
        got = m(x.cuda()).cpu()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            got16 = m(x.cuda()).float().cpu()
        with torch.autocast("cpu", dtype=torch.bfloat16):
            ref16 = ref_net(x).float()
    assert got.shape == ref.shape == (2, 2) + tuple(size) and got.dtype == torch.float32
    scale = float(ref.abs().max())
    assert float((got - ref).abs().max()) <= 1e-3 * scale
    # bf16: no worse than 1.5x the restatement's own error under CPU bf16 autocast
    err16, ref_err16 = float((got16 - ref).abs().max()), float((ref16 - ref).abs().max())
    print("bf16 max error", err16, "CPU autocast", ref_err16)
    assert err16 <= 1.5 * ref_err16, (err16, ref_err16)


def _loss(y, tgt):
    p = torch.sigmoid(y)
    dice = 1 - (2 * (p * tgt).sum() + 1e-5) / (p.sum() + tgt.sum() + 1e-5)
    return F.binary_cross_entropy_with_logits(y, tgt) + dice


@pytest.mark.parametrize("norm,pos", [("instance", "perceptron"), ("batch", "conv")])
def test_unetr_training_step_matches_torch_autograd(norm, pos):
    cfg = _cfg((32, 32, 32), 192, 3, 8, 384, norm, pos, c_out=1)
    m = _model(cfg, seed=4)
    st0 = copy.deepcopy(m.state_dict())
    ref_net = RefUNETR(m, cfg, torch.float64)         # float64: the reference's own rounding stays far below the tolerance
    x = torch.rand(2, 1, 32, 32, 32, generator=torch.Generator().manual_seed(5))
    tgt = (torch.rand(2, 1, 32, 32, 32, generator=torch.Generator().manual_seed(6)) > 0.7).float()
    ref_loss = _loss(ref_net(x.double(), training=True), tgt.double())
    ref_loss.backward()
    ref32 = RefUNETR(m, cfg)                          # torch's own fp32 autograd: the noise floor of an fp32 step
    _loss(ref32(x, training=True), tgt).backward()
    m = m.cuda().train()
    loss = _loss(m(x.cuda()), tgt.cuda())
    loss.backward()
    assert abs(float(loss.detach()) - float(ref_loss.detach())) <= 1e-4 * max(1.0, abs(float(ref_loss)))
    worst = (0.0, "", 0.0, 0.0)
    for k, p in m.named_parameters():
        r = ref_net.p[k[len("model."):]].grad
        assert p.grad is not None and r is not None, k
        rel = float((p.grad.cpu().double() - r.double()).norm() / r.double().norm().clamp_min(1e-30))
        floor = float((ref32.p[k[len("model."):]].grad.double() - r.double()).norm() / r.double().norm().clamp_min(1e-30))
        # 2e-3 relative L2 per tensor, or no worse than 1.5x torch's own fp32 autograd where cancellation makes that the floor.  Measured
        # worst: 1.3e-3, from the shared instance-norm statistics (one-pass sums), not from the ViT kernels
        worst = max(worst, (rel / max(2e-3, 1.5 * floor), k, rel, floor))
    print("worst gradient error / bound", worst)
    assert worst[0] <= 1.0, worst

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


def test_unetr_refusals_on_the_device():
    m = _model(_cfg()).cuda()
    with pytest.raises(ValueError, match="input_size"):
        with torch.no_grad():
            m.eval()(torch.rand(1, 1, 32, 32, 48).cuda())
    md = _model(_cfg(dropout=0.1)).cuda()
    with torch.no_grad():
        assert torch.isfinite(md.eval()(torch.rand(1, 1, 32, 32, 32).cuda())).all()      # eval: dropout is the identity
    with pytest.raises(NotImplementedError, match="dropout"):
        md.train()(torch.rand(1, 1, 32, 32, 32).cuda())


_GLUE = ("aten::bmm", "aten::matmul", "aten::mm", "aten::addmm", "aten::linear", "aten::softmax", "aten::_softmax", "aten::layer_norm",
         "aten::native_layer_norm", "aten::gelu", "aten::cat", "aten::scaled_dot_product_attention")


def test_unetr_runs_no_torch_glue():
    """Forward and backward of a training step run none of the aten compute ops the network would otherwise need."""
    m = _model(_cfg((32, 32, 32), 192, 3, 8, 384, "batch", "perceptron", c_out=1), seed=2).cuda().train()
    x = torch.rand(2, 1, 32, 32, 32, device="cuda")
    tgt = (torch.rand(2, 1, 32, 32, 32, device="cuda") > 0.5).float()
    F.binary_cross_entropy_with_logits(m(x), tgt).backward()          # warm-up: weight packs, library load
    torch.cuda.synchronize()
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        F.binary_cross_entropy_with_logits(m(x), tgt).backward()
        torch.cuda.synchronize()
    names = {e.key for e in prof.key_averages()}
    bad = sorted(n for n in names if n in _GLUE or n.startswith("aten::conv") or n.startswith("aten::_conv")
                 or n.startswith("aten::miopen") or n.startswith("aten::_scaled_dot") or n.startswith("aten::_flash"))
    assert not bad, bad


def test_unetr_in_sliding_window_engine():
    from pytorch_connectomics_amd.inference.window import EagerSlidingWindowEngine
    m = _model(_cfg((32, 32, 32), c_out=1), seed=9).cuda().eval()
    vol = torch.rand(1, 1, 48, 40, 64, generator=torch.Generator().manual_seed(2)).cuda()
    eng = EagerSlidingWindowEngine(roi_size=(32, 32, 32), sw_batch_size=2, overlap=0.5, mode="bump", padding_mode="constant",
                                   cval=0.0)
    with torch.no_grad():
        out = eng(vol, m)
    assert out.shape == (1, 1, 48, 40, 64) and torch.isfinite(out).all()
    # one window through the engine is the model itself
    one = torch.rand(1, 1, 32, 32, 32, generator=torch.Generator().manual_seed(4)).cuda()
    eng1 = EagerSlidingWindowEngine(roi_size=(32, 32, 32), sw_batch_size=1, overlap=0.5, mode="constant", padding_mode="constant",
                                    cval=0.0)
    with torch.no_grad():
        got = eng1(one, m)
        direct = m(one)
    torch.testing.assert_close(got, direct, rtol=1e-6, atol=1e-6)
    # two disjoint windows with constant blending: each half of the volume is the direct forward of its window
    two = torch.rand(1, 1, 32, 32, 64, generator=torch.Generator().manual_seed(6)).cuda()
    eng0 = EagerSlidingWindowEngine(roi_size=(32, 32, 32), sw_batch_size=2, overlap=0.0, mode="constant", padding_mode="constant",
                                    cval=0.0)
    with torch.no_grad():
        got = eng0(two, m)
        direct = m(torch.cat([two[..., :32], two[..., 32:]], 0))
    torch.testing.assert_close(got[..., :32], direct[:1], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(got[..., 32:], direct[1:], rtol=1e-5, atol=1e-5)


def test_cli_unetr_train_then_test(tmp_path):
    """tutorials/minimal_unetr.yaml as committed (only its output directory moved under tmp_path): trains two steps, then predicts."""
    import re
    from pathlib import Path
    from pytorch_connectomics_amd.inference.artifact import read_prediction_artifact
    from pytorch_connectomics_amd.main import main
    text = (Path(__file__).resolve().parents[1] / "tutorials" / "minimal_unetr.yaml").read_text()
    cfg = tmp_path / "minimal_unetr.yaml"
    cfg.write_text(re.sub(r"(?m)^save_path: .*$", f"save_path: {tmp_path / 'out'}", text, count=1))
    out = main(["--config", str(cfg), "--mode", "train"])
    assert out["steps"] == 2 and np.isfinite(out["first_loss"])
    ck = tmp_path / "out" / "checkpoints" / "last.ckpt"
    blob = torch.load(ck, weights_only=True)
    assert blob["global_step"] == 2
    assert "model.model.vit.blocks.11.attn.qkv.weight" in blob["state_dict"]
    assert "model.model.decoder2.conv_block.conv3.conv.weight" in blob["state_dict"]
    res = main(["--config", str(cfg), "--mode", "test", "--checkpoint", str(ck)])
    assert res["output_voxels_per_s"] > 0
    pred = read_prediction_artifact(next((tmp_path / "out" / "results").glob("*_prediction.h5")))
    assert pred.shape == (1, 80, 96, 112) and np.isfinite(pred).all() and pred.std() > 0

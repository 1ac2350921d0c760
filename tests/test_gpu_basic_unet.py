"""GPU parity of the MONAI BasicUNet (`monai_basic_unet3d`, reference monai_models.py:142-194) and of its fused UpCat kernels
(csrc/upcat_kernels.hip) against PyTorch-CPU fp32.  The CPU reference below restates monai.networks.nets.BasicUNet with torch.nn
modules of the same child names and loads the HIP model's own state_dict (MONAI itself is not installed: unpinned, like
`monai_unet`)."""
import copy
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _cl(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _cf(x):
    return x.permute(0, 4, 1, 2, 3).contiguous()


def _rel(a, r):
    return float((a.float() - r.float()).abs().max() / r.float().abs().max().clamp_min(1e-8))


# ------------------------------------------------------------------------------------------------------------ UpCat kernels
def _upcat_ref(x_e, x_low, w, b):
    """monai UpCat without its convs: deconv -> replicate pad (high end, one voxel where the skip is longer) -> cat([skip, up])."""
    x0 = F.conv_transpose3d(x_low, w, b, stride=2)
    sp = [0] * 6
    for i in range(3):
        if x_e.shape[-i - 1] != x0.shape[-i - 1]:
            sp[i * 2 + 1] = 1
    return torch.cat([x_e, F.pad(x0, sp, "replicate")], dim=1)


@pytest.mark.parametrize("skip", [(6, 8, 10), (7, 8, 10), (6, 9, 10), (6, 8, 11), (7, 9, 11)])
@pytest.mark.parametrize("c_in,c_e,c_u", [(24, 20, 12), (128, 32, 64), (13, 7, 5)])
@pytest.mark.parametrize("dt,tol", [(torch.float32, 2e-5), (torch.bfloat16, 3e-2)])
def test_upcat_matches_deconv_pad_cat(skip, c_in, c_e, c_u, dt, tol):
    from pytorch_connectomics_amd.training.rsunet_autograd import UpCatFn
    g = torch.Generator().manual_seed(c_in * 7 + c_u + sum(skip))
    low = (3, 4, 5)
    x_low = torch.randn(2, c_in, *low, generator=g).to(dt).float().requires_grad_(True)
    x_e = torch.randn(2, c_e, *skip, generator=g).to(dt).float().requires_grad_(True)
    w = (torch.randn(c_in, c_u, 2, 2, 2, generator=g) * 0.1).requires_grad_(True)
    b = torch.randn(c_u, generator=g).requires_grad_(True)
    wr = w.detach().to(dt).float().requires_grad_(True)        # the kernel's MFMA operand is the weight in the storage type
    ref = _upcat_ref(x_e, x_low, wr, b)
    gy = torch.randn(ref.shape, generator=g).to(dt).float()
    ref.backward(gy)
    xe_d = _cl(x_e.detach()).cuda().to(dt).requires_grad_(True)
    xl_d = _cl(x_low.detach()).cuda().to(dt).requires_grad_(True)
    wd = w.detach().cuda().requires_grad_(True)
    bd = b.detach().cuda().requires_grad_(True)
    y = UpCatFn.apply(xe_d, xl_d, wd, bd)
    assert tuple(y.shape) == (2,) + skip + (c_e + c_u,) and y.dtype == dt
    y.backward(_cl(gy).cuda().to(dt))
    assert _rel(_cf(y.detach().cpu()), ref.detach()) < tol
    assert torch.equal(_cf(y.detach().cpu())[:, :c_e], x_e.detach().to(dt))           # the skip half is a copy
    assert _rel(_cf(xe_d.grad.cpu()), x_e.grad) < tol
    assert _rel(_cf(xl_d.grad.cpu()), x_low.grad) < tol
    assert _rel(wd.grad.cpu(), wr.grad) < tol
    assert _rel(bd.grad.cpu(), b.grad) < tol


def test_upcat_backward_is_bit_reproducible():
    from pytorch_connectomics_amd import hip_ops as ops
    g = torch.Generator().manual_seed(1)
    x_low = torch.randn(2, 9, 10, 11, 48, generator=g).cuda().to(torch.bfloat16)
    dcat = torch.randn(2, 19, 21, 22, 40 + 24, generator=g).cuda().to(torch.bfloat16)
    w = torch.randn(48, 24, 2, 2, 2, generator=g).cuda()
    first = ops.upcat_deconv2_bwd(dcat, x_low, w, 40)
    for _ in range(2):
        again = ops.upcat_deconv2_bwd(dcat, x_low, w, 40)
        assert all(torch.equal(a, b) for a, b in zip(first, again))


# ------------------------------------------------------------------------------------------------------ CPU reference network
def _act(name):
    return {"relu": nn.ReLU, "leakyrelu": nn.LeakyReLU, "prelu": nn.PReLU, "elu": nn.ELU}[name]()


def _norm(norm, c, groups):
    if norm == "batch":
        return nn.BatchNorm3d(c)
    if norm == "instance":
        return nn.InstanceNorm3d(c)
    return nn.GroupNorm(groups, c)


class RConvolution(nn.Sequential):
    def __init__(self, ci, co, act, norm, groups):
        super().__init__()
        self.conv = nn.Conv3d(ci, co, 3, padding=1)
        self.adn = nn.Sequential()
        self.adn.add_module("N", _norm(norm, co, groups))
        self.adn.add_module("D", nn.Dropout(0.0))
        self.adn.add_module("A", _act(act))


class RTwoConv(nn.Sequential):
    def __init__(self, ci, co, *a):
        super().__init__()
        self.conv_0 = RConvolution(ci, co, *a)
        self.conv_1 = RConvolution(co, co, *a)


class RDown(nn.Sequential):
    def __init__(self, ci, co, *a):
        super().__init__()
        self.max_pooling = nn.MaxPool3d(2)
        self.convs = RTwoConv(ci, co, *a)


class RUpCat(nn.Module):
    def __init__(self, ci, cc, co, *a, halves=True):
        super().__init__()
        up = ci // 2 if halves else ci
        self.upsample = nn.Sequential()
        self.upsample.add_module("deconv", nn.ConvTranspose3d(ci, up, 2, stride=2))
        self.convs = RTwoConv(cc + up, co, *a)

    def forward(self, x, x_e):
        x0 = self.upsample(x)
        sp = [0] * 6
        for i in range(3):
            if x_e.shape[-i - 1] != x0.shape[-i - 1]:
                sp[i * 2 + 1] = 1
        return self.convs(torch.cat([x_e, F.pad(x0, sp, "replicate")], dim=1))


class RBasicUNet(nn.Module):
    def __init__(self, in_ch, out_ch, f, act, norm, groups):
        super().__init__()
        a = (act, norm, groups)
        self.conv_0 = RTwoConv(in_ch, f[0], *a)
        self.down_1, self.down_2 = RDown(f[0], f[1], *a), RDown(f[1], f[2], *a)
        self.down_3, self.down_4 = RDown(f[2], f[3], *a), RDown(f[3], f[4], *a)
        self.upcat_4, self.upcat_3 = RUpCat(f[4], f[3], f[3], *a), RUpCat(f[3], f[2], f[2], *a)
        self.upcat_2, self.upcat_1 = RUpCat(f[2], f[1], f[1], *a), RUpCat(f[1], f[0], f[5], *a, halves=False)
        self.final_conv = nn.Conv3d(f[5], out_ch, 1)

    def forward(self, x):
        x0 = self.conv_0(x)
        x1 = self.down_1(x0)
        x2 = self.down_2(x1)
        x3 = self.down_3(x2)
        x4 = self.down_4(x3)
        u = self.upcat_4(x4, x3)
        u = self.upcat_3(u, x2)
        u = self.upcat_2(u, x1)
        return self.final_conv(self.upcat_1(u, x0))


def _cfg(filters, norm="batch", act="relu", groups=2, size=(16, 16, 16), out_ch=2):
    return NS(model=NS(arch=NS(type="monai_basic_unet3d"), in_channels=1, out_channels=out_ch, input_size=list(size),
                       monai=NS(filters=list(filters), norm=norm, num_groups=groups, activation=act, dropout=0.0,
                                upsample_mode="deconv")))


def _pair(cfg, seed=0):
    """(HIP model, CPU reference holding the HIP model's state_dict) in a 'trained' state: non-trivial norm affine, running statistics
    and PReLU slopes."""
    from pytorch_connectomics_amd.models import build_model
    torch.manual_seed(seed)
    m = build_model(cfg)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("adn.N.weight") or n.endswith("adn.N.bias"):
                p.add_(0.2 * torch.randn(p.shape, generator=g))
            if n.endswith("adn.A.weight"):
                p.copy_(0.1 + 0.3 * torch.rand(p.shape, generator=g))
        for n, b in m.named_buffers():
            if n.endswith("running_mean"):
                b.copy_(0.3 * torch.randn(b.shape, generator=g))
            if n.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
    mc = cfg.model.monai
    ref = RBasicUNet(1, cfg.model.out_channels, m.model.features, mc.activation, mc.norm, mc.num_groups)
    ref.load_state_dict({k[len("model."):]: v for k, v in m.state_dict().items()}, strict=True)
    return m, ref


_F5 = (8, 16, 24, 32, 40)


@pytest.mark.parametrize("size,filters,norm,groups,act", [
    ((16, 16, 16), (8, 16), "group", 1, "relu"),              # the reference's e2e configuration
    ((16, 16, 16), (8, 16), "group", 1, "prelu"),
    ((17, 23, 30), _F5, "batch", 2, "relu"),
    ((17, 23, 30), _F5, "batch", 2, "prelu"),
    ((17, 35, 34), _F5, "instance", 2, "relu"),              # instance norm needs > 1 voxel at the bottom (1 x 2 x 2 here)
    ((17, 35, 34), _F5, "instance", 2, "prelu"),
    ((17, 23, 30), _F5, "group", 4, "relu"),
    ((17, 23, 30), _F5, "group", 4, "prelu"),
    ((17, 35, 34), _F5, "instance", 2, "leakyrelu"),
    ((16, 16, 16), _F5, "batch", 2, "elu"),
])
def test_basic_unet_forward_matches_torch(size, filters, norm, groups, act):
    cfg = _cfg(filters, norm, act, groups, size)
    m, ref_net = _pair(cfg)
    x = torch.rand(2, 1, *size, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        ref = ref_net.eval()(x)
        m = m.cuda().eval()
        got = m(x.cuda()).cpu()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            got16 = m(x.cuda()).float().cpu()
    assert got.shape == ref.shape == (2, 2) + tuple(size) and got.dtype == torch.float32
    torch.testing.assert_close(got, ref, rtol=1e-3, atol=1e-3 * float(ref.abs().max()))
    assert (torch.sigmoid(got16) - torch.sigmoid(ref)).abs().max() < 6e-2


def _train_step(m, x, tgt):
    loss = F.binary_cross_entropy_with_logits(m(x), tgt)
    loss.backward()
    return loss


def test_basic_unet_training_step_matches_torch_autograd():
    cfg = _cfg(_F5, "batch", "relu", size=(17, 23, 30), out_ch=1)
    m, ref_net = _pair(cfg, seed=4)
    st0 = copy.deepcopy(m.state_dict())
    x = torch.rand(2, 1, 17, 23, 30, generator=torch.Generator().manual_seed(5))
    tgt = (torch.rand(2, 1, 17, 23, 30, generator=torch.Generator().manual_seed(6)) > 0.7).float()
    ref_loss = _train_step(ref_net.train(), x, tgt)
    m = m.cuda().train()
    loss = _train_step(m, x.cuda(), tgt.cuda())
    assert abs(float(loss.detach()) - float(ref_loss.detach())) < 1e-4
    named_ref = dict(ref_net.named_parameters())
    g, r = [], []
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        g.append(p.grad.cpu().flatten().double())
        r.append(named_ref[k[len("model."):]].grad.flatten().double())
    g, r = torch.cat(g), torch.cat(r)
    cos = float((g * r).sum() / (g.norm() * r.norm()))
    rel2 = float((g - r).norm() / r.norm())
    assert cos > 0.99995 and rel2 < 1e-2, (cos, rel2)
    sd = m.state_dict()
    for k in ("model.conv_0.conv_0.adn.N", "model.upcat_1.convs.conv_1.adn.N"):
        torch.testing.assert_close(sd[k + ".running_mean"].cpu(), ref_net.state_dict()[k[6:] + ".running_mean"], rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(sd[k + ".running_var"].cpu(), ref_net.state_dict()[k[6:] + ".running_var"], rtol=1e-4, atol=1e-5)
        assert not torch.equal(sd[k + ".running_mean"].cpu(), st0[k + ".running_mean"])
        assert int(sd[k + ".num_batches_tracked"]) == 1

    # two identical optimizer steps from the same state: bit-equal parameters and buffers
    def step():
        m.load_state_dict(st0)
        opt = torch.optim.SGD(m.parameters(), lr=0.1)
        opt.zero_grad(set_to_none=True)
        _train_step(m, x.cuda(), tgt.cuda())
        opt.step()
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in m.state_dict().items()}
    a, b = step(), step()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_basic_unet_refusals_on_the_device():
    m, _ = _pair(_cfg((8, 16)))
    m = m.cuda()
    with pytest.raises(ValueError, match="axis H"):
        with torch.no_grad():
            m.eval()(torch.rand(1, 1, 16, 15, 16).cuda())
    cfg = _cfg((8, 16))
    cfg.model.monai.dropout = 0.1
    md, _ = _pair(cfg)
    md = md.cuda()
    with torch.no_grad():
        assert torch.isfinite(md.eval()(torch.rand(1, 1, 16, 16, 16).cuda())).all()      # eval: dropout is the identity
    with pytest.raises(NotImplementedError, match="dropout"):
        md.train()(torch.rand(1, 1, 16, 16, 16).cuda())


def test_basic_unet_runs_no_torch_glue():
    """Forward and backward of the network run none of aten::cat / replication_pad3d / conv* on the device."""
    m, _ = _pair(_cfg(_F5, "batch", "relu", size=(17, 23, 30), out_ch=1), seed=2)
    m = m.cuda().train()
    x = torch.rand(2, 1, 17, 23, 30, device="cuda")
    tgt = (torch.rand(2, 1, 17, 23, 30, device="cuda") > 0.5).float()
    _train_step(m, x, tgt)                         # warm-up: weight packs, library load
    torch.cuda.synchronize()
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        _train_step(m, x, tgt)
        torch.cuda.synchronize()
    names = {e.key for e in prof.key_averages()}
    bad = sorted(n for n in names if n in ("aten::cat", "aten::replication_pad3d")
                 or n.startswith("aten::conv") or n.startswith("aten::_conv") or n.startswith("aten::cudnn")
                 or n.startswith("aten::miopen"))
    assert not bad, bad


def test_basic_unet_in_sliding_window_engine():
    from pytorch_connectomics_amd.inference.window import EagerSlidingWindowEngine
    m, _ = _pair(_cfg((8, 16), "batch", "relu", size=(16, 32, 32), out_ch=1), seed=9)
    m = m.cuda().eval()
    vol = torch.rand(1, 1, 24, 56, 64, generator=torch.Generator().manual_seed(2)).cuda()
    eng = EagerSlidingWindowEngine(roi_size=(16, 32, 32), sw_batch_size=2, overlap=0.5, mode="bump", padding_mode="constant",
                                   cval=0.0)
    outs = {}
    for n in (1, 2):
        eng.pipeline_streams = n
        with torch.no_grad():
            outs[n] = eng(vol, m)
        torch.cuda.synchronize()
        assert eng.last_stats["streams"] == n
    assert torch.equal(outs[1], outs[2])
    # one window through the engine is the model itself
    one = torch.rand(1, 1, 16, 32, 32, generator=torch.Generator().manual_seed(4)).cuda()
    eng1 = EagerSlidingWindowEngine(roi_size=(16, 32, 32), sw_batch_size=1, overlap=0.5, mode="constant", padding_mode="constant",
                                    cval=0.0)
    with torch.no_grad():
        got = eng1(one, m)
        direct = m(one)
    torch.testing.assert_close(got, direct, rtol=1e-6, atol=1e-6)


def test_cli_basic_unet_train_then_test(tmp_path):
    from pytorch_connectomics_amd.inference.artifact import read_prediction_artifact
    from pytorch_connectomics_amd.main import main
    cfg = tmp_path / "basic.yaml"
    cfg.write_text(f"""
experiment_name: basic_unet_demo
save_path: {tmp_path / 'out'}
default:
  optimization: {{precision: "32"}}
  model:
    arch: {{type: monai_basic_unet3d}}
    in_channels: 1
    out_channels: 1
    input_size: [32, 64, 64]
    output_size: [32, 64, 64]
    monai: {{filters: [8, 16], norm: group, num_groups: 1, dropout: 0.0}}
    loss:
      losses:
        - {{function: DiceLoss, weight: 1.0, pred_slice: "0:1", target_slice: "0:1"}}
  data:
    train: {{image: "random://basic/train_image", label: "random://basic/train_label"}}
    dataloader: {{batch_size: 1, patch_size: [32, 64, 64]}}
    image_transform: {{normalize: none}}
  inference:
    window: {{window_size: [32, 64, 64], overlap: 0.5, sw_batch_size: 2}}
    model: {{channel_activations: [{{channels: ":", activation: sigmoid}}]}}
train:
  optimization:
    max_epochs: 1
    n_steps_per_epoch: 1
    precision: "32"
    optimizer: {{name: AdamW, lr: 1.0e-4}}
  system: {{seed: 42}}
test:
  data:
    test: {{image: "random://basic/test_image?shape=40,96,80"}}
""")
    out = main(["--config", str(cfg), "--mode", "train"])
    assert out["steps"] == 1 and np.isfinite(out["first_loss"])
    ck = tmp_path / "out" / "checkpoints" / "last.ckpt"
    blob = torch.load(ck, weights_only=True)
    # the Lightning layout prefixes the wrapper's keys (model.conv_0. ...) with the module attribute "model."
    assert blob["global_step"] == 1 and any(k.startswith("model.model.conv_0.") for k in blob["state_dict"])
    assert "model.model.conv_0.conv_0.conv.weight" in blob["state_dict"] and "model.model.upcat_1.upsample.deconv.weight" in blob["state_dict"]
    res = main(["--config", str(cfg), "--mode", "test", "--checkpoint", str(ck)])
    assert res["output_voxels_per_s"] > 0
    pred = read_prediction_artifact(next((tmp_path / "out" / "results").glob("*_prediction.h5")))
    assert pred.shape == (1, 40, 96, 80) and 0.0 <= pred.min() and pred.max() <= 1.0 and pred.std() > 0

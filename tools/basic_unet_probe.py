"""Probe of `monai_basic_unet3d` on one MI355X: bf16 forward per window batch, training step (forward + BCE + backward), and an A/B of
the fused UpCat kernel against the composition the older kernels allow.  Prints one JSON line.

    python tools/basic_unet_probe.py [--batch 2] [--size 64 128 128] [--iters 20] [--ab-rounds 30]

Workload: default filters (32, 64, 128, 256, 512) -> (..., 512, 512), batch 2, 1 x 64 x 128 x 128, batch norm, ReLU.
A/B, per upcat_* shape (forward only, the two alternated round by round, device events, median):
    fused    ops.upcat_deconv2_fwd: the concat buffer written once by the GEMM's scatter epilogue + the skip copy
    compose  conv3d_strided (gather-form ConvTranspose3d k2 / s2 / p0, out_dims = 2 d) -> F.pad(replicate) where the skip is longer
             -> torch.cat -- a measurement of what the older kernels allow, never a product path
Algorithmic bytes of the fused forward: x_low + x_e + W (fp32) read, cat written; achieved bytes/s = those bytes over the median time.
Under `rocprofv3 --kernel-trace --stats` (--profile-only: a few iterations, no A/B) the per-kernel times come from the trace.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path
from types import SimpleNamespace as NS

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def _events_ms(fn, iters: int, warmup: int = 3) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def _compose(ops, x_low, wpack, bias, x_e, c_u):
    up = ops.conv3d_strided(x_low, wpack, c_out=c_u, kernel=(2, 2, 2), stride=(2, 2, 2), pad=(0, 0, 0),
                            out_dims=tuple(2 * int(d) for d in x_low.shape[1:4]), transposed=True, bias=bias)
    sp = [0] * 6
    for i in range(3):
        if x_e.shape[3 - i] != up.shape[3 - i]:
            sp[i * 2 + 1] = 1
    if any(sp):
        up = F.pad(up.permute(0, 4, 1, 2, 3), sp, "replicate").permute(0, 2, 3, 4, 1)
    return torch.cat([x_e, up], dim=-1)


def upcat_ab(model, batch: int, size, rounds: int) -> dict:
    from pytorch_connectomics_amd import hip_ops as ops
    net = model.model
    f = net.features
    dt = torch.bfloat16
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    res = {}
    levels = [("upcat_4", 4, 3), ("upcat_3", 3, 2), ("upcat_2", 2, 1), ("upcat_1", 1, 0)]
    for name, lo, hi in levels:
        m = getattr(net, name)
        w = m.upsample.deconv.weight.detach().float().contiguous()
        b = m.upsample.deconv.bias.detach().float().contiguous()
        c_in, c_u = int(w.shape[0]), int(w.shape[1])
        c_e = f[hi]
        low = [int(s) >> lo for s in size]
        skip = [int(s) >> hi for s in size]
        x_low = torch.randn(batch, *low, c_in, device=dev, generator=g).to(dt)
        x_e = torch.randn(batch, *skip, c_e, device=dev, generator=g).to(dt)
        wpack = ops.conv3d_pack_weight_direct(w, dt, layout="convT")
        a = ops.upcat_deconv2_fwd(x_low, w, b, x_e)
        c = _compose(ops, x_low, wpack, b, x_e, c_u)
        diff = float((a.float() - c.float()).abs().max())
        dcat = torch.randn_like(a)
        ta, tb, tbw = [], [], []
        for _ in range(3):
            ops.upcat_deconv2_fwd(x_low, w, b, x_e)
            _compose(ops, x_low, wpack, b, x_e, c_u)
            ops.upcat_deconv2_bwd(dcat, x_low, w, c_e)
        torch.cuda.synchronize()
        for _ in range(rounds):
            for fn, out in ((lambda: ops.upcat_deconv2_fwd(x_low, w, b, x_e), ta),
                            (lambda: _compose(ops, x_low, wpack, b, x_e, c_u), tb),
                            (lambda: ops.upcat_deconv2_bwd(dcat, x_low, w, c_e), tbw)):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                fn()
                e.record()
                torch.cuda.synchronize()
                out.append(s.elapsed_time(e))
        rows = batch * low[0] * low[1] * low[2]
        vox = batch * skip[0] * skip[1] * skip[2]
        fwd_bytes = 2 * (rows * c_in + vox * c_e + vox * (c_e + c_u)) + 4 * w.numel()
        # backward: dcat read (skip half once, up half by both GEMMs), x_low read, dx_e + dx_low written, dW partials ignored
        bwd_bytes = 2 * (vox * c_e * 2 + 2 * vox * c_u + rows * c_in * 2 + rows * c_in)
        fa, fb, fbw = statistics.median(ta), statistics.median(tb), statistics.median(tbw)
        res[name] = dict(x_low=[batch, *low, c_in], x_e=[batch, *skip, c_e], c_u=c_u, fused_fwd_ms=round(fa, 4),
                         compose_fwd_ms=round(fb, 4), speedup=round(fb / fa, 3), fused_bwd_ms=round(fbw, 4),
                         fwd_bytes=fwd_bytes, fwd_GBps=round(fwd_bytes / fa / 1e6, 1),
                         fwd_TFLOPs=round(2 * rows * c_in * 8 * c_u / fa / 1e9, 2),
                         bwd_bytes_min=bwd_bytes, bwd_GBps=round(bwd_bytes / fbw / 1e6, 1),
                         fused_vs_compose_max_abs=diff,
                         spread_fused=[round(min(ta), 4), round(max(ta), 4)], spread_compose=[round(min(tb), 4), round(max(tb), 4)])
    return res


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, nargs=3, default=[64, 128, 128])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--ab-rounds", type=int, default=30)
    ap.add_argument("--profile-only", action="store_true", help="a few forward / training iterations for a kernel trace, no A/B")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("basic_unet_probe needs an MI355X: there is no CPU measurement")
    from pytorch_connectomics_amd.models import build_model
    cfg = NS(model=NS(arch=NS(type="monai_basic_unet3d"), in_channels=1, out_channels=1, input_size=list(args.size),
                      monai=NS(filters=[32, 64, 128, 256, 512], norm="batch", activation="relu", dropout=0.0, upsample_mode="deconv")))
    torch.manual_seed(0)
    model = build_model(cfg).cuda()
    x = torch.rand(args.batch, 1, *args.size, device="cuda")
    tgt = (torch.rand(args.batch, 1, *args.size, device="cuda") > 0.5).float()
    iters = 3 if args.profile_only else args.iters

    model.eval()

    def fwd():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            model(x)

    fwd_ms = _events_ms(fwd, iters)
    model.train()

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = F.binary_cross_entropy_with_logits(model(x), tgt)
        loss.backward()
        for p in model.parameters():
            p.grad = None

    train_ms = _events_ms(step, iters)
    out = dict(arch="monai_basic_unet3d", filters=list(model.model.features), batch=args.batch, size=list(args.size),
               bf16_forward_ms_per_window_batch=round(fwd_ms, 3), bf16_train_fwd_bwd_ms_per_step=round(train_ms, 3), iters=iters)
    if not args.profile_only:
        out["upcat_ab"] = upcat_ab(model, args.batch, args.size, args.ab_rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

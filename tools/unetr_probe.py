"""Probe of `monai_unetr` on one MI355X: forward and training step of the default-width network, and the attention kernel alone
against torch.nn.functional.scaled_dot_product_attention on the same shapes (a comparison only; SDPA is never on the product path).

    python tools/unetr_probe.py [--batch 2] [--size 96] [--iters 10] [--out profiles/unetr_probe.txt]

Workload: default UNETR (feature_size 16, hidden 768, mlp 3072, 12 heads of 64, perceptron, instance norm), 1 -> 1 channels, batch 2,
size^3 input, bf16 autocast.  Attention shapes: N = 216 (96^3) and 512 (128^3) tokens, 12 heads of 64, bf16, forward and backward.
Device-event timing, median of `iters` rounds.  Under `rocprofv3 --kernel-trace --stats` (--profile-only) the per-kernel times come
from the trace.
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


def _median_ms(fn, iters: int, warmup: int = 3) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    return statistics.median(times)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "unetr_probe.txt"))
    a = ap.parse_args(argv)
    from pytorch_connectomics_amd.models import build_model
    from pytorch_connectomics_amd.training.transformer_autograd import AttentionFn
    dev = torch.device("cuda")
    torch.manual_seed(0)
    cfg = NS(model=NS(arch=NS(type="monai_unetr"), in_channels=1, out_channels=1, input_size=[a.size] * 3, transformer=NS()))
    m = build_model(cfg).to(dev)
    x = torch.rand(a.batch, 1, a.size, a.size, a.size, device=dev)
    tgt = (torch.rand_like(x) > 0.7).float()
    iters = 2 if a.profile_only else a.iters

    def fwd():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            m.eval()(x)

    def step():
        m.train()
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = m(x)
        F.binary_cross_entropy_with_logits(y, tgt).backward()

    res = {"workload": f"monai_unetr default widths, batch {a.batch}, 1x{a.size}^3, bf16", "forward_ms": _median_ms(fwd, iters),
           "train_step_ms": _median_ms(step, iters), "attention": []}
    for n in (216, 512):
        heads, d = 12, 64
        qkv = torch.randn(a.batch * n, 3 * heads * d, device=dev, dtype=torch.bfloat16, requires_grad=True)
        do = torch.randn(a.batch * n, heads * d, device=dev, dtype=torch.bfloat16)
        q4 = qkv.detach().reshape(a.batch, n, 3, heads, d).permute(2, 0, 3, 1, 4).contiguous().requires_grad_(True)
        do4 = do.reshape(a.batch, n, heads, d).permute(0, 2, 1, 3).contiguous()

        def hip_f():
            AttentionFn.apply(qkv, a.batch, heads)

        def hip_fb():
            AttentionFn.apply(qkv, a.batch, heads).backward(do)

        def sdpa_f():
            F.scaled_dot_product_attention(q4[0], q4[1], q4[2])

        def sdpa_fb():
            F.scaled_dot_product_attention(q4[0], q4[1], q4[2]).backward(do4)

        with torch.no_grad():
            r = {"N": n, "heads": heads, "d_head": d, "batch": a.batch, "hip_fwd_us": 1e3 * _median_ms(hip_f, iters),
                 "sdpa_fwd_us": 1e3 * _median_ms(sdpa_f, iters)}
        r["hip_fwd_bwd_us"] = 1e3 * _median_ms(hip_fb, iters)
        r["sdpa_fwd_bwd_us"] = 1e3 * _median_ms(sdpa_fb, iters)
        res["attention"].append(r)
    line = json.dumps(res)
    print(line)
    if not a.profile_only:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(__doc__.split("\n\n")[0] + "\n\n" + json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

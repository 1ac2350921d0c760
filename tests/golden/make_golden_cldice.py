"""Generate tests/golden/soft_cldice.npz from the REFERENCE's own SoftClDiceLoss (run in the build container only).

    python tests/golden/make_golden_cldice.py

Drives connectomics/models/losses/losses.py:47-85, :456-721 (through tests/golden/_ref_shim.py, as make_golden.py's losses_extra
does) on the seeded cases of tests/cldice_cases.py and stores inputs, loss values, input gradients, skeletons and error messages, and
the reference LossOrchestrator's value and gradient for the `loss_soft_cldice` profile term (no mask).
"""
from __future__ import annotations

import sys
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import _ref_shim as S  # noqa: E402
from cldice_cases import CASES, ERRORS, SKELETONS, case_tensors, skeleton_input  # noqa: E402


def main():
    ls = S.ref("connectomics.models.losses.losses")
    out = {}
    for name in sorted(CASES):
        kwargs = CASES[name][0]
        pred, target, weight = case_tensors(name)
        x = pred.clone().requires_grad_(True)
        v = ls.SoftClDiceLoss(**kwargs)(x, target, weight=weight)
        (g,) = torch.autograd.grad(v.sum(), x)
        out[f"{name}__pred"], out[f"{name}__target"] = pred.numpy(), target.numpy()
        if weight is not None:
            out[f"{name}__weight"] = weight.numpy()
        out[f"{name}__loss"] = v.detach().numpy().astype(np.float32)
        out[f"{name}__grad"] = g.numpy()
        print(name, v.detach().flatten().tolist())
    for name in sorted(SKELETONS):
        x, n = skeleton_input(name)
        out[f"skel_{name}__x"] = x.numpy()
        out[f"skel_{name}__s"] = ls._soft_skeletonize_pool(x, n).numpy()
    for name, (kwargs, p, t, w) in ERRORS.items():
        try:
            loss = ls.SoftClDiceLoss(**kwargs)
            if p is not None:
                loss(p(), t(), weight=None if w is None else w())
            msg = ""
        except ValueError as e:
            msg = str(e)
        assert msg, name
        out[f"err__{name}"] = np.asarray(msg)
    # the reference orchestrator on the loss_soft_cldice profile term (config/profiles/loss_profiles.yaml), no mask: the
    # class-balancing weight map reaches the loss as `weight` (metadata.py:46)
    S._stub_pkg("connectomics.training.losses")
    S._stub_pkg("connectomics.config.pipeline")
    meta = S.ref("connectomics.models.losses.metadata")
    ml = sys.modules["connectomics.models.losses"]
    for n in dir(meta):
        if not n.startswith("_"):
            setattr(ml, n, getattr(meta, n))
    orch = S.ref("connectomics.training.losses.orchestrator")
    for label, kw, N in (("orch_profile", {"mode": "binary", "num_iters": 5, "sigmoid": True}, 2),
                         ("orch_none_single", {"mode": "binary", "num_iters": 2, "sigmoid": True, "reduction": "none"}, 1),
                         ("orch_none_batch", {"mode": "binary", "num_iters": 2, "sigmoid": True, "reduction": "none"}, 2)):
        terms = [{"function": "SoftClDiceLoss", "weight": 1.0, "kwargs": kw}]
        cfg = NS(model=NS(loss=NS(deep_supervision=False, deep_supervision_weights=[1.0], deep_supervision_clamp_min=-20.0,
                                  deep_supervision_clamp_max=20.0, losses=terms, loss_balancing=None),
                          primary_head=None, heads=None, out_channels=1), data=NS(label_transform=None))
        o = orch.LossOrchestrator(cfg, torch.nn.ModuleList([ls.SoftClDiceLoss(**kw)]), [1.0], enable_nan_detection=True,
                                  debug_on_nan=False, resolve_affinity_mode_fn=lambda c: None)
        g = torch.Generator().manual_seed(6000 + N)
        logits = torch.randn(N, 1, 9, 10, 11, generator=g) * 8.0                 # beyond the +-20 clamp in places
        labels = (torch.rand(N, 1, 9, 10, 11, generator=g) > 0.7).float()
        out[f"{label}__logits"], out[f"{label}__labels"] = logits.numpy(), labels.numpy()
        x = logits.clone().requires_grad_(True)
        try:
            total, _ = o.compute_standard_loss(x, labels, stage="train", mask=None)
            total.sum().backward()
            out[f"{label}__total"] = total.detach().numpy().astype(np.float64)
            out[f"{label}__grad"] = x.grad.numpy()
            print(label, total.detach().flatten().tolist())
        except RuntimeError as e:
            out[f"{label}__error"] = np.asarray(f"{type(e).__name__}: {e}")
            print(label, "error:", e)
    np.savez_compressed(HERE / "soft_cldice.npz", **out)
    print("wrote soft_cldice.npz", len(out), "arrays")


if __name__ == "__main__":
    main()

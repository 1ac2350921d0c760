"""Generate tests/golden/scnp.npz from the REFERENCE's own ScnpLoss (run in the build container only).

    python tests/golden/make_golden_scnp.py

Drives connectomics/models/losses/losses.py:354-453 (through tests/golden/_ref_shim.py, as make_golden_cldice.py does) on the seeded
cases of tests/scnp_cases.py and stores inputs, the neighbour-penalised logits, loss values, input gradients and error messages, and
the reference LossOrchestrator's value and gradient for a ScnpLoss term without a mask (logits beyond the +-20 clamp).
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
from scnp_cases import CASES, ERRORS, case_tensors  # noqa: E402


def main():
    ls = S.ref("connectomics.models.losses.losses")
    out = {}
    for name in sorted(CASES):
        kwargs = CASES[name][0]
        logits, target, weight = case_tensors(name)
        loss = ls.ScnpLoss(**kwargs)
        x = logits.clone().requires_grad_(True)
        # the reference slices its weight per channel: a one-channel weight reaches it expanded
        v = loss(x, target, weight=None if weight is None else weight.expand_as(x))
        (g,) = torch.autograd.grad(v, x)
        out[f"{name}__logits"], out[f"{name}__target"] = logits.numpy(), target.numpy()
        if weight is not None:
            out[f"{name}__weight"] = weight.numpy()
        out[f"{name}__z"] = loss._scnp_logits(logits, target).numpy()
        out[f"{name}__loss"] = v.detach().numpy().astype(np.float32)
        out[f"{name}__grad"] = g.numpy()
        print(name, float(v.detach()))
    for name, kwargs in ERRORS.items():
        try:
            ls.ScnpLoss(**kwargs)
            msg = ""
        except ValueError as e:
            msg = str(e)
        assert msg, name
        out[f"err__{name}"] = np.asarray(msg)
    try:
        ls.ScnpLoss()(torch.zeros(2, 5, 5), torch.zeros(2, 5, 5))
        raise AssertionError("3-D logits were accepted")
    except ValueError as e:
        out["err__logits_3d"] = np.asarray(str(e))
    # the reference orchestrator on a ScnpLoss term, no mask: the class-balancing weight map reaches the loss as `weight`
    # (metadata.py:45), the logits are clamped to +-20 first
    S._stub_pkg("connectomics.training.losses")
    S._stub_pkg("connectomics.config.pipeline")
    meta = S.ref("connectomics.models.losses.metadata")
    ml = sys.modules["connectomics.models.losses"]
    for n in dir(meta):
        if not n.startswith("_"):
            setattr(ml, n, getattr(meta, n))
    orch = S.ref("connectomics.training.losses.orchestrator")
    kw = {"neighborhood_size": 3}
    terms = [{"function": "ScnpLoss", "weight": 1.0, "kwargs": kw}]
    cfg = NS(model=NS(loss=NS(deep_supervision=False, deep_supervision_weights=[1.0], deep_supervision_clamp_min=-20.0,
                              deep_supervision_clamp_max=20.0, losses=terms, loss_balancing=None),
                      primary_head=None, heads=None, out_channels=3), data=NS(label_transform=None))
    o = orch.LossOrchestrator(cfg, torch.nn.ModuleList([ls.ScnpLoss(**kw)]), [1.0], enable_nan_detection=True, debug_on_nan=False,
                              resolve_affinity_mode_fn=lambda c: None)
    g = torch.Generator().manual_seed(8002)
    logits = torch.randn(2, 3, 7, 9, 11, generator=g) * 12.0                     # beyond the +-20 clamp in places
    labels = (torch.rand(2, 3, 7, 9, 11, generator=g) > 0.7).float()
    out["orch__logits"], out["orch__labels"] = logits.numpy(), labels.numpy()
    x = logits.clone().requires_grad_(True)
    total, _ = o.compute_standard_loss(x, labels, stage="train", mask=None)
    total.backward()
    out["orch__total"] = total.detach().numpy().astype(np.float64)
    out["orch__grad"] = x.grad.numpy()
    print("orch", float(total.detach()))
    np.savez_compressed(HERE / "scnp.npz", **out)
    print("wrote scnp.npz", len(out), "arrays")


if __name__ == "__main__":
    main()

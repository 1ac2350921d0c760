"""Generate tests/golden/softmax_losses.npz from the REFERENCE's own code (run in the build container only).

    python tests/golden/make_golden_softmax_losses.py

Drives connectomics/models/losses/losses.py:88-137 (CrossEntropyLossWrapper, through tests/golden/_ref_shim.py, as
make_golden_scnp.py does) on the seeded cases of tests/softmax_loss_cases.py and stores inputs, loss values, input gradients and the
messages torch gives for the refused arguments; then the reference's LossOrchestrator on a CrossEntropyLoss term with logits beyond
the +-20 clamp, a batch mask and two deep-supervision scales (nearest-resized class-index targets): totals and every output's gradient.
"""
from __future__ import annotations

import sys
import warnings
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import _ref_shim as S  # noqa: E402
import softmax_loss_cases as SC  # noqa: E402


def main():
    warnings.filterwarnings("ignore")
    ls = S.ref("connectomics.models.losses.losses")
    out = {}
    for name in sorted(SC.CE_CASES):
        logits, target = SC.ce_case_tensors(name)
        x = logits.clone().requires_grad_(True)
        v = ls.CrossEntropyLossWrapper(**SC.ce_kwargs(name))(x, target)
        (g,) = torch.autograd.grad(v, x)
        out[f"{name}__logits"], out[f"{name}__target"] = logits.numpy(), target.numpy()
        out[f"{name}__loss"], out[f"{name}__grad"] = v.detach().numpy().astype(np.float32), g.numpy()
        print(name, float(v.detach()))
    for name, (kwargs, C) in SC.CE_ERRORS.items():
        kw = {k: (torch.tensor(v) if k == "weight" else v) for k, v in kwargs.items()}
        try:
            ls.CrossEntropyLossWrapper(**kw)(torch.zeros(1, C, 2, 3, 4), torch.zeros(1, 1, 2, 3, 4))
            msg = ""
        except (ValueError, RuntimeError) as e:
            msg = str(e)
        assert msg, name
        out[f"err__{name}"] = np.asarray(msg)
        print(name, msg)
    # the reference's planner and orchestrator
    S._stub_pkg("connectomics.training.losses")
    S._stub_pkg("connectomics.config.pipeline")
    meta = S.ref("connectomics.models.losses.metadata")
    ml = sys.modules["connectomics.models.losses"]
    for n in dir(meta):
        if not n.startswith("_"):
            setattr(ml, n, getattr(meta, n))
    orch = S.ref("connectomics.training.losses.orchestrator")
    for which, ds in (("ds", True), ("plain", False)):
        mods = torch.nn.ModuleList([meta.attach_loss_metadata(ls.CrossEntropyLossWrapper(**dict(t.get("kwargs", {}))), t["function"])
                                    for t in SC.ORCH_TERMS])
        o = orch.LossOrchestrator(SC.orch_cfg(ds), mods, [float(t["weight"]) for t in SC.ORCH_TERMS], enable_nan_detection=True,
                                  debug_on_nan=False, resolve_affinity_mode_fn=lambda c: None)
        outs, labels, mask = SC.orch_tensors()
        if not ds:
            outs = {"output": outs["output"]}
        outs = {k: v.clone().requires_grad_(True) for k, v in outs.items()}
        if ds:
            total, _ = o.compute_deep_supervision_loss(outs, labels, stage="train", mask=mask)
        else:
            total, _ = o.compute_standard_loss(outs["output"], labels, stage="train", mask=mask)
        total.backward()
        out[f"orch_{which}__total"] = np.float64(total.item())
        for k, v in outs.items():
            out[f"orch_{which}__in_{k}"], out[f"orch_{which}__grad_{k}"] = v.detach().numpy(), v.grad.numpy().copy()
        out[f"orch_{which}__labels"], out[f"orch_{which}__mask"] = labels.numpy(), mask.numpy()
        out[f"orch_{which}__plan"] = np.asarray([f"{t.call_kind}|{t.target_kind}|{t.spatial_weight_arg}|{t.target_slice}" for t in o.loss_term_specs])
        print("orch", which, float(total.detach()), list(out[f"orch_{which}__plan"]))
    np.savez_compressed(HERE / "softmax_losses.npz", **out)
    print("wrote softmax_losses.npz", len(out), "arrays", (HERE / "softmax_losses.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()

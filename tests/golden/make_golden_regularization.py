"""Generate tests/golden/regularization.npz from the REFERENCE's own regularisation losses (run in the build container only).

    python tests/golden/make_golden_regularization.py

Drives connectomics/models/losses/regularization.py (through tests/golden/_ref_shim.py, as make_golden_scnp.py does) on the seeded
cases of tests/regularization_cases.py and stores inputs, masks, loss values, the gradient of every input and the error messages;
then the reference's LossOrchestrator (training/losses/orchestrator.py, plan.py, models/losses/metadata.py) on three term lists: a
`pred_only` and a `pred_pred` term with `mask_slice` next to supervised terms, named heads with `pred2_head` across heads, and
deep supervision with `apply_deep_supervision: false` on one term -- totals and the gradient of every output.
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
from regularization_cases import CASES, ERRORS, ORCH_TERMS, case_tensors, orch_cfg, orch_tensors  # noqa: E402


def main():
    warnings.filterwarnings("ignore")
    reg = S.ref("connectomics.models.losses.regularization")
    out = {}
    for name in sorted(CASES):
        loss_name, kwargs = CASES[name][:2]
        inputs, mask = case_tensors(name)
        xs = [t.clone().requires_grad_(True) for t in inputs]
        loss = getattr(reg, loss_name)(**kwargs)
        v = loss(*xs) if mask is None else loss(*xs, mask=mask)
        grads = torch.autograd.grad(v, xs)
        for k, (t, g) in enumerate(zip(inputs, grads)):
            out[f"{name}__in{k}"], out[f"{name}__grad{k}"] = t.numpy(), g.numpy()
        if mask is not None:
            out[f"{name}__mask"] = mask.numpy()
        out[f"{name}__loss"] = v.detach().numpy().astype(np.float32)
        print(name, float(v.detach()))
    for name, (loss_name, kwargs, shapes) in ERRORS.items():
        try:
            getattr(reg, loss_name)(**kwargs)(*[torch.zeros(s) for s in shapes])
            msg = ""
        except ValueError as e:
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
    ls = S.ref("connectomics.models.losses.losses")
    orch = S.ref("connectomics.training.losses.orchestrator")
    make = {"WeightedBCEWithLogitsLoss": ls.WeightedBCEWithLogitsLoss, "WeightedMSELoss": ls.WeightedMSELoss}
    make.update({n: getattr(reg, n) for n in reg.__all__})
    for which in sorted(ORCH_TERMS):
        terms = ORCH_TERMS[which]
        mods = torch.nn.ModuleList([meta.attach_loss_metadata(make[t["function"]](**dict(t.get("kwargs", {}))), t["function"]) for t in terms])
        o = orch.LossOrchestrator(orch_cfg(which), mods, [float(t.get("coefficient", t.get("weight", 1.0))) for t in terms],
                                  enable_nan_detection=True, debug_on_nan=False, resolve_affinity_mode_fn=lambda c: None)
        outs, labels, mask = orch_tensors(which)
        outs = {k: v.clone().requires_grad_(True) for k, v in outs.items()}
        if which == "deep_supervision":
            total, _ = o.compute_deep_supervision_loss(outs, labels, stage="train", mask=mask)
        elif which == "heads":
            total, _ = o.compute_standard_loss(dict(outs), labels, stage="train", mask=mask)
        else:
            total, _ = o.compute_standard_loss(outs["output"], labels, stage="train", mask=mask)
        total.backward()
        out[f"orch_{which}__total"] = np.float64(total.item())
        for k, v in outs.items():
            out[f"orch_{which}__in_{k}"], out[f"orch_{which}__grad_{k}"] = v.detach().numpy(), v.grad.numpy().copy()
        out[f"orch_{which}__labels"], out[f"orch_{which}__mask"] = labels.numpy(), mask.numpy()
        # the plan the reference compiled: call kind, spatial argument and the second slice / head of every term
        out[f"orch_{which}__plan"] = np.asarray([f"{t.call_kind}|{t.spatial_weight_arg}|{t.pred_slice}|{t.pred2_slice}|{t.pred2_head}|"
                                                 f"{t.mask_slice}|{t.apply_deep_supervision}" for t in o.loss_term_specs])
        print("orch", which, float(total.detach()), list(out[f"orch_{which}__plan"]))
    np.savez_compressed(HERE / "regularization.npz", **out)
    print("wrote regularization.npz", len(out), "arrays", (HERE / "regularization.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()

"""CPU tests of ScnpLoss (training/scnp_autograd.py) against tests/golden/scnp.npz, which the reference's own ScnpLoss and
LossOrchestrator wrote (tests/golden/make_golden_scnp.py): the torch restatement's neighbour-penalised logits (bit for bit), values
and input gradients for every case, the error messages, and the term through ConnectomicsModule."""
import sys
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from scnp_cases import CASES, ERRORS  # noqa: E402

GOLD = Path(__file__).parent / "golden"


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD / "scnp.npz")


def _case(g, name):
    weight = torch.from_numpy(g[f"{name}__weight"]) if f"{name}__weight" in g.files else None
    return torch.from_numpy(g[f"{name}__logits"]), torch.from_numpy(g[f"{name}__target"]), weight


@pytest.mark.parametrize("name", sorted(CASES))
def test_restated_logits_are_the_reference_logits(gold, name):
    from pytorch_connectomics_amd.training.scnp_autograd import scnp_logits_torch
    x, t, _ = _case(gold, name)
    assert torch.equal(scnp_logits_torch(x, t, CASES[name][0]["neighborhood_size"]), torch.from_numpy(gold[f"{name}__z"]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_reference_values_and_gradients(gold, name):
    from pytorch_connectomics_amd.training.scnp_autograd import ScnpLoss
    logits, target, weight = _case(gold, name)
    x = logits.clone().requires_grad_(True)
    v = ScnpLoss(**CASES[name][0])(x, target, weight=weight)
    (grad,) = torch.autograd.grad(v, x)
    assert v.dim() == 0
    assert torch.allclose(v.detach(), torch.from_numpy(gold[f"{name}__loss"]), rtol=1e-5, atol=0), name
    gw = torch.from_numpy(gold[f"{name}__grad"])
    assert torch.allclose(grad, gw, rtol=1e-5, atol=1e-6 * float(gw.abs().max())), name


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_constructor_errors_match_reference_messages(gold, name):
    from pytorch_connectomics_amd.training.scnp_autograd import ScnpLoss
    with pytest.raises(ValueError) as e:
        ScnpLoss(**ERRORS[name])
    assert str(e.value) == str(gold[f"err__{name}"])


def test_input_rank_error_matches_reference_message(gold):
    from pytorch_connectomics_amd.training.scnp_autograd import ScnpLoss, scnp_logits_torch
    with pytest.raises(ValueError) as e:
        ScnpLoss()(torch.zeros(2, 5, 5), torch.zeros(2, 5, 5))
    assert str(e.value) == str(gold["err__logits_3d"])
    with pytest.raises(ValueError) as e:
        scnp_logits_torch(torch.zeros(2, 5, 5), torch.zeros(2, 5, 5), 3)
    assert str(e.value) == str(gold["err__logits_3d"])


def test_non_scalar_reduction_is_refused_by_name():
    from pytorch_connectomics_amd.training.scnp_autograd import ScnpLoss
    with pytest.raises(ValueError, match="ScnpLoss reduction must be 'mean' or 'sum', got 'none'"):
        ScnpLoss(reduction="none")


def test_hip_backend_refuses_cpu_tensors():
    from pytorch_connectomics_amd.training.scnp_autograd import ScnpLoss
    x = torch.rand(1, 1, 5, 5, 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ScnpLoss(use_hip=True)(x, x)


def test_cpu_path_takes_any_odd_size():
    from pytorch_connectomics_amd.training.scnp_autograd import ScnpLoss
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, 1, 12, 12, 12, generator=g)
    assert torch.isfinite(ScnpLoss(neighborhood_size=9)(x, (x > 0.3).float()))


def test_constant_same_class_logits_give_the_per_channel_bce():
    """The identity the reference's unit test states: when all voxels of a class share one logit the pooling changes nothing."""
    from pytorch_connectomics_amd.training.module import per_channel_bce_with_logits
    from pytorch_connectomics_amd.training.scnp_autograd import ScnpLoss
    g = torch.Generator().manual_seed(0)
    target = (torch.rand(2, 3, 8, 8, 8, generator=g) > 0.5).float()
    logits = torch.where(target > 0.5, 4.0, -4.0)
    for auto in (False, True):
        a = ScnpLoss(neighborhood_size=3, auto_pos_weight=auto)(logits, target)
        assert torch.allclose(a, per_channel_bce_with_logits(logits, target, auto_pos_weight=auto), rtol=1e-6, atol=0)


def _cfg(kwargs):
    return NS(model=NS(loss=NS(deep_supervision=False, deep_supervision_weights=[1.0], deep_supervision_clamp_min=-20.0,
                               deep_supervision_clamp_max=20.0, losses=[{"function": "ScnpLoss", "weight": 1.0, "kwargs": kwargs}],
                               loss_balancing=None, fused=True), primary_head=None, heads=None, out_channels=3),
              data=NS(label_transform=None), optimization=NS())


def test_module_term_matches_reference_orchestrator(gold):
    from pytorch_connectomics_amd.training.module import ConnectomicsModule
    m = ConnectomicsModule(_cfg({"neighborhood_size": 3}), model=torch.nn.Identity())
    x = torch.from_numpy(gold["orch__logits"]).requires_grad_(True)
    total, parts = m._compute_loss(x, torch.from_numpy(gold["orch__labels"]))
    total.backward()
    assert float(total.detach()) == pytest.approx(float(gold["orch__total"]), rel=1e-5)
    gw = torch.from_numpy(gold["orch__grad"])
    assert torch.allclose(x.grad, gw, rtol=1e-5, atol=1e-6 * float(gw.abs().max()))
    assert "loss_0_ScnpLoss" in parts


def test_term_list_with_scnp_is_not_fusable():
    from pytorch_connectomics_amd.training.module import ConnectomicsModule
    cfg = _cfg({})
    cfg.model.loss.losses.insert(0, {"function": "WeightedBCEWithLogitsLoss", "weight": 1.0})
    m = ConnectomicsModule(cfg, model=torch.nn.Identity())
    pred = torch.zeros(1, 3, 4, 4, 4)
    assert m._term_is_fusable(m.loss_terms[0], pred) and not m._term_is_fusable(m.loss_terms[1], pred)


def test_constructor_errors_surface_when_the_module_is_built():
    from pytorch_connectomics_amd.training.module import ConnectomicsModule
    with pytest.raises(ValueError, match="neighborhood_size must be a positive odd int, got 4"):
        ConnectomicsModule(_cfg({"neighborhood_size": 4}), model=torch.nn.Identity())

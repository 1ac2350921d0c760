"""Shared by tests/golden/make_golden_scnp.py (the REFERENCE's ScnpLoss runs them) and the ScnpLoss tests: seeded inputs and
constructor arguments.  Every volume holds at most a few thousand voxels."""
import torch

S3, S2 = (2, 3, 7, 9, 11), (2, 2, 13, 10)

# name: (kwargs, shape, logits kind, target kind, weight kind)
#   logits kind: random (sigma 4) | int (rounded to integers: heavy ties) | bf16 (rounded to the bf16 grid) | huge (+-2e4, unclamped:
#                the supplier of a window can be of the other class, the gradient there is 0)
#   target kind: binary | soft (values in {0, 0.3, 0.7, 1}: the class gate at 0.5 and the counts at 0 disagree) | no_fg (channel 0 has
#                no foreground) | all_fg (channel 0 is all foreground) | rare (n_neg / n_pos exceeds max_pos_weight)
#   weight kind: None | full (C channels, a zero region and non-unit values) | one (1 channel: this package's path only; the
#                reference's class cannot slice it and sees it expanded)
CASES = {
    "d3_ns1": ({"neighborhood_size": 1}, S3, "random", "binary", None),
    "d3_ns3": ({"neighborhood_size": 3}, S3, "random", "binary", None),
    "d3_ns5": ({"neighborhood_size": 5}, S3, "random", "binary", "full"),
    "d3_ns7": ({"neighborhood_size": 7}, S3, "random", "binary", None),
    "d2_ns1": ({"neighborhood_size": 1}, S2, "random", "binary", "full"),
    "d2_ns3": ({"neighborhood_size": 3}, S2, "random", "binary", None),
    "d2_ns5": ({"neighborhood_size": 5}, S2, "random", "binary", None),
    "d2_ns7": ({"neighborhood_size": 7}, S2, "random", "binary", "full"),
    "ties_int_ns3": ({"neighborhood_size": 3}, S3, "int", "binary", "full"),
    "ties_int_ns5": ({"neighborhood_size": 5}, S3, "int", "binary", None),
    "ties_int_d2_ns7": ({"neighborhood_size": 7}, S2, "int", "binary", None),
    "ties_bf16_ns3": ({"neighborhood_size": 3}, S3, "bf16", "binary", None),
    "ties_bf16_d2_ns5": ({"neighborhood_size": 5}, S2, "bf16", "soft", "full"),
    "no_foreground_channel": ({"neighborhood_size": 3}, S3, "random", "no_fg", None),
    "all_foreground_channel": ({"neighborhood_size": 3}, S3, "random", "all_fg", "full"),
    "capped_pos_weight": ({"neighborhood_size": 3, "max_pos_weight": 4.0}, S3, "random", "rare", None),
    "soft_targets": ({"neighborhood_size": 3}, S3, "random", "soft", "full"),
    "weight_full": ({"neighborhood_size": 3}, S3, "random", "binary", "full"),
    "weight_one_channel": ({"neighborhood_size": 3}, S3, "int", "soft", "one"),
    "no_auto_pos_weight": ({"neighborhood_size": 3, "auto_pos_weight": False}, S3, "random", "binary", "full"),
    "reduction_sum": ({"neighborhood_size": 3, "reduction": "sum"}, S3, "random", "binary", "full"),
    "reduction_sum_d2_int": ({"neighborhood_size": 5, "reduction": "sum"}, S2, "int", "binary", None),
    "window_wider_than_volume": ({"neighborhood_size": 5}, (1, 1, 1, 30, 4), "int", "binary", None),
    "huge_logits": ({"neighborhood_size": 3}, S3, "huge", "binary", "full"),
}


def case_tensors(name: str):
    """(logits, target, weight) of a case, float32 on the CPU."""
    kwargs, shape, lk, tk, wk = CASES[name]
    g = torch.Generator().manual_seed(7000 + sorted(CASES).index(name))
    N, C = shape[:2]
    sp = shape[2:]
    x = torch.randn(shape, generator=g) * 4.0
    if lk == "int":
        x = x.round()
    elif lk == "bf16":
        x = x.to(torch.bfloat16).float()
    elif lk == "huge":
        x = torch.where(torch.rand(shape, generator=g) < 0.3, torch.sign(x) * 2.0e4, x)
    r = torch.rand(shape, generator=g)
    if tk == "soft":
        target = torch.tensor([0.0, 0.3, 0.7, 1.0])[torch.randint(0, 4, shape, generator=g)]
    elif tk == "rare":
        target = (r > 0.97).float()
    else:
        target = (r > 0.6).float()
        if tk == "no_fg":
            target[:, 0] = 0.0
        elif tk == "all_fg":
            target[:, 0] = 1.0
    if wk is None:
        weight = None
    else:
        wshape = shape if wk == "full" else (N, 1, *sp)
        weight = (torch.rand(wshape, generator=g) * 2.0 + 0.25) * (torch.rand(wshape, generator=g) > 0.25).float()
        weight[..., :3] = 0.0                          # a zero region
    return x, target, weight


# constructor errors of the reference: name -> kwargs
ERRORS = {"even_size": {"neighborhood_size": 2}, "zero_size": {"neighborhood_size": 0}, "negative_size": {"neighborhood_size": -3}}

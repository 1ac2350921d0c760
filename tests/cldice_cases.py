"""Shared by tests/golden/make_golden_cldice.py (the REFERENCE's SoftClDiceLoss runs them) and the SoftClDiceLoss tests: seeded
inputs, constructor arguments and the error cases of the reference's checks."""
import torch

# name: (kwargs, pred shape, pred kind, target kind, weight kind)
#   pred kind:   logits | prob | plateau_logits (saturated +-25 and 0, clamped to +-20 first) | binary_prob (exact 0 / 1)
#                | loose_prob (slightly outside [0, 1]: clamp_probabilities)
#   target kind: dense (same channels) | index (one channel of class indices) | dense_soft (values in [0, 1])
#   weight kind: None | fg1 (one channel, with zeros) | all (prediction channels) | neg (one channel, some negative values)
CASES = {
    "bin_sigmoid_n5": ({"num_iters": 5, "sigmoid": True}, (2, 1, 9, 10, 11), "logits", "dense", None),
    "bin_sigmoid_weight": ({"num_iters": 5, "sigmoid": True}, (2, 1, 9, 10, 11), "logits", "dense", "fg1"),
    "bin_raw_n0_sum": ({"num_iters": 0, "reduction": "sum"}, (2, 1, 8, 9, 10), "prob", "dense_soft", None),
    "bin_raw_n1_none_fgch": ({"num_iters": 1, "reduction": "none", "foreground_channel": 1}, (2, 2, 8, 9, 10), "prob", "dense", "all"),
    "multi_softmax_index": ({"num_iters": 5, "mode": "multi", "softmax": True}, (2, 3, 8, 9, 10), "logits", "index", "fg1"),
    "multi_softmax_none": ({"num_iters": 3, "mode": "multi", "softmax": True, "reduction": "none", "background_index": -1},
                           (2, 3, 8, 9, 7), "logits", "dense", "all"),
    "multi_one_channel": ({"num_iters": 2, "mode": "multi", "sigmoid": True, "smooth": 0.5}, (1, 1, 7, 8, 9), "logits", "dense", None),
    "clamp_probabilities": ({"num_iters": 5, "clamp_probabilities": True}, (2, 1, 8, 9, 10), "loose_prob", "dense_soft", "neg"),
    "plateau_sigmoid": ({"num_iters": 5, "sigmoid": True}, (2, 1, 9, 10, 11), "plateau_logits", "dense", "fg1"),
    "plateau_binary_prob": ({"num_iters": 5}, (2, 1, 9, 10, 11), "binary_prob", "dense", None),
    "two_d_sigmoid": ({"num_iters": 5, "sigmoid": True}, (2, 1, 17, 19), "logits", "dense", "fg1"),
    "two_d_plateau_multi": ({"num_iters": 4, "mode": "multi", "softmax": True}, (2, 3, 16, 15), "plateau_logits", "index", None),
}


def case_tensors(name: str):
    """(pred, target, weight) of a case, float32 on the CPU; pred is the raw input of the loss (logits or probabilities)."""
    kwargs, shape, pk, tk, wk = CASES[name]
    g = torch.Generator().manual_seed(4000 + sorted(CASES).index(name))
    N, C = shape[:2]
    sp = shape[2:]
    if pk == "logits":
        pred = torch.randn(shape, generator=g) * 3.0
    elif pk == "prob":
        pred = torch.rand(shape, generator=g)
    elif pk == "plateau_logits":
        r = torch.rand(shape, generator=g)
        pred = torch.where(r > 0.55, torch.full(shape, 25.0), torch.where(r < 0.3, torch.full(shape, -25.0), torch.zeros(shape)))
        pred = pred.clamp(-20.0, 20.0)                 # what the training module hands the loss
    elif pk == "binary_prob":
        pred = (torch.rand(shape, generator=g) > 0.4).float()
    else:                                             # loose_prob
        pred = torch.rand(shape, generator=g) * 1.2 - 0.1
    if tk == "index":
        target = torch.randint(0, C, (N, 1, *sp), generator=g).float()
    elif tk == "dense_soft":
        target = torch.rand(shape, generator=g)
    else:
        target = (torch.rand(shape, generator=g) > 0.6).float()
    if wk is None:
        weight = None
    elif wk == "fg1":
        weight = torch.rand((N, 1, *sp), generator=g) * 2.0 * (torch.rand((N, 1, *sp), generator=g) > 0.2).float()
    elif wk == "all":
        weight = torch.rand(shape, generator=g) + 0.5
    else:                                             # neg
        weight = torch.rand((N, 1, *sp), generator=g) * 2.0 - 0.3
    return pred, target, weight


# skeleton fixtures: name -> (shape, kind, num_iters)
SKELETONS = {
    "rand5_n0": ((2, 1, 9, 10, 11), "prob", 0),
    "rand5_n1": ((2, 1, 9, 10, 11), "prob", 1),
    "rand5_n5": ((2, 2, 9, 10, 11), "prob", 5),
    "plateau5_n5": ((2, 1, 9, 10, 11), "binary_prob", 5),
    "rand4_n5": ((2, 2, 17, 19), "prob", 5),
}


def skeleton_input(name: str):
    shape, kind, n = SKELETONS[name]
    g = torch.Generator().manual_seed(5000 + sorted(SKELETONS).index(name))
    x = torch.rand(shape, generator=g)
    return ((x > 0.4).float() if kind == "binary_prob" else x), n


# error cases: name -> (constructor kwargs, pred, target, weight) -- pred etc. are zero-argument builders (None: constructor error)
def _t(*shape, fill=0.5):
    return lambda: torch.full(shape, float(fill))


ERRORS = {
    "ctor_num_iters": ({"num_iters": -1}, None, None, None),
    "ctor_mode": ({"mode": "dual"}, None, None, None),
    "ctor_reduction": ({"reduction": "max"}, None, None, None),
    "ctor_smooth": ({"smooth": 0.0}, None, None, None),
    "ctor_both_activations": ({"sigmoid": True, "softmax": True}, None, None, None),
    "ctor_tolerance": ({"validation_tolerance": -1.0}, None, None, None),
    "pred_3d": ({}, _t(2, 5, 5), _t(2, 5, 5), None),
    "softmax_one_channel": ({"softmax": True}, _t(1, 1, 4, 4, 4), _t(1, 1, 4, 4, 4), None),
    "target_ndim": ({}, _t(1, 1, 4, 4, 4), _t(4, 4), None),
    "target_shape": ({}, _t(1, 1, 4, 4, 4), _t(1, 1, 4, 4, 5), None),
    "target_channels": ({}, _t(1, 3, 4, 4, 4), _t(1, 2, 4, 4, 4), None),
    "class_index_range": ({"mode": "multi"}, _t(1, 3, 4, 4, 4), _t(1, 1, 4, 4, 4, fill=3), None),
    "spatial_too_small": ({}, _t(1, 1, 4, 2, 4), _t(1, 1, 4, 2, 4), None),
    "pred_range": ({}, _t(1, 1, 4, 4, 4, fill=1.5), _t(1, 1, 4, 4, 4), None),
    "target_range": ({}, _t(1, 1, 4, 4, 4), _t(1, 1, 4, 4, 4, fill=-0.5), None),
    "foreground_channel": ({"foreground_channel": 4}, _t(1, 3, 4, 4, 4), _t(1, 3, 4, 4, 4), None),
    "background_index": ({"mode": "multi", "background_index": 5}, _t(1, 3, 4, 4, 4), _t(1, 3, 4, 4, 4), None),
    "weight_ndim": ({}, _t(1, 1, 4, 4, 4), _t(1, 1, 4, 4, 4), _t(4, 4)),
    "weight_shape": ({}, _t(1, 1, 4, 4, 4), _t(1, 1, 4, 4, 4), _t(1, 1, 4, 4, 3)),
    "weight_channels": ({"mode": "multi"}, _t(1, 4, 4, 4, 4), _t(1, 4, 4, 4, 4), _t(1, 2, 4, 4, 4)),
}

"""`decoding.steps` of a configuration -> the one decoder call this engine runs (the reference's decoding/pipeline.py
normalize_decode_modes + apply_decode_pipeline, for a single step)."""
from __future__ import annotations

from typing import Any, Mapping, Optional, Tuple

from .registry import get_decoder, list_decoders


def _get(node: Any, key: str, default=None):
    if isinstance(node, Mapping):
        return node.get(key, default)
    return getattr(node, key, default)


def plan_decoding(cfg) -> Optional[Tuple[str, dict]]:
    """(decoder name, kwargs) of the configured decoding, or None when `decoding` is absent, `enabled: false` or has no enabled step.
    A step names its decoder as `name` (or `function_name`) and its arguments as `kwargs`.  A step this engine does not build, or more
    than one step, is a NotImplementedError that names it."""
    dec = _get(cfg, "decoding")
    if dec is None or not bool(_get(dec, "enabled", True)):
        return None
    steps = [s for s in (_get(dec, "steps") or []) if bool(_get(s, "enabled", True))]
    if not steps:
        return None
    names = [_get(s, "name") or _get(s, "function_name") for s in steps]
    if any(not n for n in names):
        raise ValueError("Decode step is missing required field 'name'.")
    built = list_decoders()
    for n in names:
        if n not in built:
            raise NotImplementedError(f"decoding step '{n}' is not built by this engine (built: {built}); watershed, mutex watershed, "
                                      "the binary / contour / distance decoders and the branch / merge tools stay with the reference")
    if len(names) > 1:
        raise NotImplementedError(f"decoding.steps {names}: a chain of steps is not built, a single step of {built} is")
    kwargs = _get(steps[0], "kwargs") or {}
    return names[0], {str(k): v for k, v in dict(kwargs).items()}


def run_decoding(cfg, prediction):
    """Run the configured decoding step on a prediction (C, Z, Y, X): a device tensor gives the int32 device labels, a numpy array the
    compact numpy labels.  None when nothing is configured."""
    plan = plan_decoding(cfg)
    if plan is None:
        return None
    name, kwargs = plan
    return get_decoder(name)(prediction, **kwargs)

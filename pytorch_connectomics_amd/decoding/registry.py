"""Name -> decoder registry with the reference's function names (decoding/registry.py:82-101).  It holds the decoders this engine
builds; the reference registers its whole library here, this one a single entry."""
from __future__ import annotations

from typing import Callable, Dict, List

_DECODERS: Dict[str, Callable] = {}


def register_decoder(name: str, fn: Callable, *, overwrite: bool = False) -> None:
    if not name or not isinstance(name, str):
        raise ValueError("Decoder name must be a non-empty string.")
    if not callable(fn):
        raise TypeError(f"Decoder '{name}' must be callable.")
    existing = _DECODERS.get(name)
    if existing is not None and not overwrite and existing is not fn:
        raise ValueError(f"Decoder '{name}' already registered. Use overwrite=True to replace it.")
    _DECODERS[name] = fn


def get_decoder(name: str) -> Callable:
    try:
        return _DECODERS[name]
    except KeyError as exc:
        raise KeyError(f"Unknown decoder '{name}'. Available decoders: [{', '.join(sorted(_DECODERS))}]") from exc


def list_decoders() -> List[str]:
    return sorted(_DECODERS)

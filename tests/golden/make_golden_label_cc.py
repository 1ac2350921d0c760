"""Generate tests/golden/label_cc.npz from the REFERENCE's own apply_decoding_postprocessing (run in the build container only).

    python tests/golden/make_golden_label_cc.py

Drives connectomics/decoding/stage.py apply_decoding_postprocessing through tests/golden/_ref_shim.py.  cc3d is not installed here, so a
stand-in `cc3d` module is registered whose connected_components and dust are the scipy model of tests/label_cc_cases.py: what the
fixture pins is therefore the WRAPPER -- the `enabled` gate, `instance_cc3d` counting whenever it is not None, an empty node giving
connectivity 6 and min_size 0, the first sample of a 4-D input with the axis put back, the transpose applied last and a bad one keeping
the shape -- and not cc3d's numbering or dust rule, which stay stated from memory (tests/label_cc_cases.py).

Stored per case: `<name>__ids` (the int32 input), `<name>__cfg` (the configuration as JSON text), `<name>__out` (what the reference
function returned).  Data only.
"""
from __future__ import annotations

import json
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))
import _ref_shim as S  # noqa: E402
import label_cc_cases as L  # noqa: E402


def _stand_in_cc3d():
    mod = types.ModuleType("cc3d")

    def connected_components(data, connectivity=26, out_dtype=None, **_):
        labels = L.model(np.asarray(data).astype(np.int64), int(connectivity))[0]
        return labels.astype(out_dtype or np.uint32)

    def dust(img, threshold, connectivity=26, in_place=False, **_):
        labels = L.model(np.asarray(img).astype(np.int64), int(connectivity))[0]
        sizes = np.bincount(labels.ravel())
        return np.where(sizes[labels] < threshold, 0, img).astype(np.asarray(img).dtype)

    mod.connected_components, mod.dust = connected_components, dust
    return mod


def _reference():
    S.install()
    S._stub_pkg("connectomics.decoding")
    sys.modules.setdefault("cc3d", _stand_in_cc3d())
    return S.ref("connectomics.decoding.stage")


def configs():
    ids = L.blocky((6, 9, 11), seed=3, n_ids=3, block=(2, 2, 3))
    post = lambda **kw: {"decoding": {"postprocessing": kw}}          # noqa: E731
    return {
        "absent": (ids, {"decoding": {}}),
        "disabled": (ids, post(enabled=False, instance_cc3d={"connectivity": 26, "min_size": 4})),
        "enabled_nothing": (ids, post(enabled=True)),
        "empty_node": (ids, post(enabled=True, instance_cc3d={})),
        "c26_dust": (ids, post(enabled=True, instance_cc3d={"connectivity": 26, "min_size": 7})),
        "c18": (ids, post(enabled=True, instance_cc3d={"connectivity": 18})),
        "four_d": (np.stack([ids, ids[::-1]]), post(enabled=True, instance_cc3d={"connectivity": 6, "min_size": 5})),
        "transpose": (ids, post(enabled=True, instance_cc3d={"connectivity": 6, "min_size": 5}, output_transpose=[2, 0, 1])),
        "transpose_only": (ids, post(enabled=True, output_transpose=[1, 0, 2])),
        "bad_transpose": (ids, post(enabled=True, instance_cc3d={"connectivity": 6}, output_transpose=[0, 1])),
    }


def main():
    stage = _reference()
    out = {}
    for name, (ids, cfg) in configs().items():
        got = stage.apply_decoding_postprocessing(cfg, ids.copy())
        out[f"{name}__ids"] = ids
        out[f"{name}__cfg"] = np.asarray(json.dumps(cfg))
        out[f"{name}__out"] = np.ascontiguousarray(got)
        print(name, ids.shape, "->", got.shape, got.dtype, "max", int(got.max()))
    np.savez_compressed(HERE / "label_cc.npz", **out)
    print("wrote label_cc.npz", len(out), "arrays", (HERE / "label_cc.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()

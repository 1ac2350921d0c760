"""Generate tests/golden/affinity_cc.npz from the REFERENCE's own serial kernel (run in the build container only).

    python tests/golden/make_golden_affinity_cc.py

Drives connectomics/decoding/decoders/segmentation_kernels.py connected_components_affinity_3d_numba through tests/golden/_ref_shim.py
on the thresholded inputs of the small cases of tests/affinity_cc_cases.py (`golden_names()`).  Without numba the kernel's `jit` is the
module's own pass-through decorator and the function runs as plain Python, which is why the stored cases stay below ~20^3 voxels.  The
module imports fastremap at its top and uses it in none of the functions called here: an empty stand-in module is registered for it.

Stored per case: `<name>__hard` (the (3, A0, A1, A2) thresholded input as packed bits), `<name>__shape`, `<name>__edge_offset`,
`<name>__seg` (the kernel's uint32 ids).  Data only.
"""
from __future__ import annotations

import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import _ref_shim as S  # noqa: E402
from affinity_cc_cases import CASES, golden_names, hard_of  # noqa: E402


def _reference():
    S.install()
    for name in ("connectomics.decoding", "connectomics.decoding.decoders"):
        S._stub_pkg(name)
    if "fastremap" not in sys.modules:
        sys.modules["fastremap"] = types.ModuleType("fastremap")
    return S.ref("connectomics.decoding.decoders.segmentation_kernels")


def main():
    kernels = _reference()
    out = {}
    for name in golden_names():
        case = CASES[name]()
        hard = hard_of(case["aff"], case["threshold"], case["channels"])
        seg = kernels.connected_components_affinity_3d_numba(hard, edge_offset=int(case["edge_offset"]))
        assert seg.dtype == np.uint32 and seg.shape == hard.shape[1:]
        out[f"{name}__hard"] = np.packbits(hard.reshape(-1))
        out[f"{name}__shape"] = np.asarray(hard.shape[1:], dtype=np.int32)
        out[f"{name}__edge_offset"] = np.asarray(case["edge_offset"], dtype=np.int32)
        out[f"{name}__seg"] = seg
        print(name, hard.shape[1:], "e", case["edge_offset"], "K", int(seg.max()))
    np.savez_compressed(HERE / "affinity_cc.npz", **out)
    print("wrote affinity_cc.npz", len(out), "arrays", (HERE / "affinity_cc.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()

"""Decoding of predictions to instances on the MI355X.  Built: `decode_affinity_cc` (connected components of the thresholded affinity
graph, csrc/cc_kernels.hip).  The reference's other decoders (watershed, mutex watershed, binary / contour / distance, the branch and
merge tools) stay with the reference: `run_decoding` refuses them by name.  `decoding.postprocessing` (instance_cc3d, output_transpose)
runs on hip_ops.label_cc (postprocess.py, csrc/label_cc_kernels.hip)."""
from .affinity_cc import compact_labels, decode_affinity_cc, seg_dtype
from .pipeline import plan_decoding, run_decoding
from .postprocess import apply_decoding_postprocessing, plan_postprocessing
from .registry import get_decoder, list_decoders, register_decoder

__all__ = ["apply_decoding_postprocessing", "compact_labels", "decode_affinity_cc", "get_decoder", "list_decoders", "plan_decoding",
           "plan_postprocessing", "register_decoder", "run_decoding", "seg_dtype"]

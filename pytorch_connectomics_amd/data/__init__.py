"""Training data on the device: targets built from instance labels by HIP kernels (label_targets.py)."""
from .label_targets import LabelTargetTransform, device_target_batches, labels_to_int32

__all__ = ["LabelTargetTransform", "device_target_batches", "labels_to_int32"]

"""Training data on the device: targets built from instance labels (label_targets.py) and the training augmentations (augment.py), both
by HIP kernels."""
from .augment import AugmentationPlan, augmented_batches
from .label_targets import LabelTargetTransform, device_target_batches, labels_to_int32, relabelled_batches

__all__ = ["AugmentationPlan", "LabelTargetTransform", "augmented_batches", "device_target_batches", "labels_to_int32",
           "relabelled_batches"]

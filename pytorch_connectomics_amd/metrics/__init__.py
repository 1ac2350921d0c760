"""Instance-segmentation metrics on the MI355X: adapted Rand error, variation of information and instance matching, the reference's
metrics/segmentation_numpy.py, computed from one label-pair table built on the device (csrc/pair_table_kernels.hip).  `finalize` holds
the plain host functions that turn the table's integer record and match list into the reference's numbers."""
from .finalize import (adapted_rand_from_record, matching_from_record, maximum_matching_size, voi_from_record)
from .segmentation import (INSTANCE_METRIC_NAMES, adapted_rand, instance_matching, instance_matching_simple, instance_metrics, voi)

__all__ = ["INSTANCE_METRIC_NAMES", "adapted_rand", "adapted_rand_from_record", "instance_matching", "instance_matching_simple",
           "instance_metrics", "matching_from_record", "maximum_matching_size", "voi", "voi_from_record"]

"""Device-side input pipeline: the reference's host augmentation chain as HIP kernels + a small host planner."""
from .augment import (AugmentHyp, DeviceAugmenter, plan_train_sample, polygon_masks, resample_segments, train_labels,  # noqa: F401
                      val_labels)
from .loader import DeviceAugmentLoader  # noqa: F401

"""Device-side input pipeline: the reference's host augmentation chain as HIP kernels + a small host planner."""
from .augment import (AugmentHyp, DeviceAugmenter, plan_train_sample, polygon_masks, resample_segments, train_labels,  # noqa: F401
                      val_labels)
from .dataset import check_det_dataset, read_labels, set_rectangle  # noqa: F401
from .loader import DeviceAugmentLoader, DeviceValLoader, build_train_loader, build_val_loader  # noqa: F401

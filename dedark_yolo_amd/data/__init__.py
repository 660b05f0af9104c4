"""Device-side input pipeline: the reference's host augmentation chain as HIP kernels + a small host planner."""
from .augment import (AugmentHyp, ClassifyHyp, DeviceAugmenter, center_crop_rect, plan_cls_sample, plan_train_sample,  # noqa: F401
                      polygon_masks, resample_segments, train_labels, val_labels)
from .dataset import check_cls_dataset, check_det_dataset, image_folder, read_labels, set_rectangle  # noqa: F401
from .loader import (ClassifyTrainLoader, ClassifyValLoader, DeviceAugmentLoader, DeviceValLoader, build_cls_train_loader,  # noqa: F401
                     build_cls_val_loader, build_train_loader, build_val_loader)

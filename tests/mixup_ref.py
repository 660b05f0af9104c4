"""Host statement of the MixUp pixels (ultralytics/data/augment.py:281-285) and the seeded cases shared by
tests/golden/make_mixup_golden.py (which runs the reference on them) and the tests (which run the product on the same inputs).
TEST INFRASTRUCTURE: the render below is oracle/augment.py's pieces plus the three-line blend."""
import numpy as np

from augtask_data import COCO_FLIP_IDX, synth_task_dataset


def blend(img1, img2, r):
    """numpy's `(img1 * r + img2 * (1 - r)).astype(np.uint8)` on two uint8 images: float64 products, float64 sum, truncation"""
    a = img1.astype(np.float64) * np.float64(r)
    b = img2.astype(np.float64) * (1.0 - float(r))
    return (a + b).astype(np.uint8)


def canvas(plan, ims):
    """what one side of a plan hands to cv2.warpAffine: the mosaic canvas, or the letterboxed image"""
    from oracle import augment as oa
    if plan.mosaic:
        return oa.mosaic4_canvas(plan.imgsz, plan.rects, [ims[i] for i in plan.sources])
    return oa.letterbox(ims[plan.sources[0]], (plan.imgsz, plan.imgsz))


def warped(plan, ims):
    from oracle import augment as oa
    return oa.cv_warp_affine_linear_u8(canvas(plan, ims), plan.M[:2], plan.size)


def render(plan, ims, hsv=True):
    """the reference's chain on the host for a plan of plan_train_sample: warp, MixUp blend when the plan carries a partner, RandomHSV
    (`hsv=False`: left out, as the golden generator's identity cvtColor / LUT stand-ins do), flips, Format -> uint8 [3, s, s] RGB"""
    from oracle import augment as oa
    img = warped(plan, ims)
    if plan.mix is not None:
        img = blend(img, warped(plan.mix, ims), plan.mix_r)
    if hsv and plan.hsv_gains is not None:
        img = oa.random_hsv(img, plan.hsv_gains)
    if plan.flipud:
        img = np.flipud(img)
    if plan.fliplr:
        img = np.fliplr(img)
    return oa.format_img(img)


# tag: (kind, imgsz, number of images, indices of images without instances, picks, hyper-parameter overrides, mask_ratio, flip_idx)
MIX_CASES = {
    "d0": ("detect", 96, 6, (), [0, 3], dict(mixup=1.0, flipud=0.5, degrees=10.0, shear=2.0), 4, None),
    "d1": ("detect", 64, 8, (1, 4, 6), [1, 4, 0, 6, 2, 1, 5, 4, 6, 3], dict(mixup=0.5, mosaic=0.5, flipud=0.5), 4, None),
    "s0": ("segment", 64, 6, (), [0, 4], dict(mixup=1.0, flipud=0.5, degrees=10.0), 1, None),
    "s1": ("segment", 64, 8, (1, 4, 6), [1, 4, 0, 6, 2, 5], dict(mixup=0.5, mosaic=0.5, flipud=0.5), 1, None),
    "p0": ("pose", 64, 6, (), [2, 5], dict(mixup=1.0, flipud=0.5, degrees=10.0), 4, COCO_FLIP_IDX),
    "p1": ("pose", 64, 8, (1, 4, 6), [1, 4, 0, 6, 2, 1, 5, 4, 6, 3], dict(mixup=0.5, mosaic=0.5, flipud=0.5), 4, COCO_FLIP_IDX),
}
FILES = dict(detect="g24_mixup.npz", segment="g24_mixseg.npz", pose="g24_mixpose.npz")


def mix_dataset(seed, tag):
    """decoded BGR images at their load_image size (long side == imgsz, so the letterbox path applies) with labels of the case's kind;
    the four low bits of every pixel are zero (the recorded canvases compress to half).  detect: the boxes of a pose dataset."""
    kind, imgsz, n_img, empty = MIX_CASES[tag][:4]
    ims, labels = synth_task_dataset(seed, n_img, imgsz, "segment" if kind == "segment" else "pose", fixed_long_side=True, empty=empty)
    ims = [im & np.uint8(0xF0) for im in ims]
    if kind == "detect":
        labels = [dict(cls=l["cls"], bboxes=l["bboxes"]) for l in labels]
    return ims, labels

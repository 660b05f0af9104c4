"""Host side of test-time augmentation for detect (predict(augment=True)): the pass geometry of tta_plan against the reference's
arithmetic (scale_img, _clip_augmented), the cfg key, the C-ABI declarations and the argument checks that need no GPU."""
import os
import re

import pytest
import torch

from util import ROOT, load_yaml

# (H, W, strides) -> (padded pass sizes, A_i, dropped tail of pass 0, dropped head of the last pass, merged A): the reference's
# scale_img (torch_utils.py:270-279) and _clip_augmented (tasks.py:331-340) evaluated by hand
TABLE = [
    ((640, 640, (8, 16, 32)), [(640, 640), (544, 544), (448, 448)], [8400, 6069, 4116], 400, 3136, 15049),
    ((128, 128, (8, 16, 32)), [(128, 128), (128, 128), (96, 96)], [336, 336, 189], 16, 144, 701),
    ((96, 160, (8, 16, 32)), [(96, 160), (96, 160), (96, 128)], [315, 315, 252], 15, 192, 675),
    ((128, 192, (8, 16, 32, 64)), [(128, 192)] * 3, [510, 510, 510], 6, 384, 1140),
    ((640, 640, (4, 8, 16, 32)), [(640, 640), (544, 544), (448, 448)], [34000, 24565, 16660], 400, 12544, 62281),
    ((64, 64, (8, 16, 32)), [(64, 64)] * 3, [84, 84, 84], 4, 64, 184),
]


@pytest.mark.parametrize("case", TABLE, ids=[f"{c[0][0]}x{c[0][1]}_nl{len(c[0][2])}_s{c[0][2][0]}" for c in TABLE])
def test_tta_plan_reproduces_the_reference_arithmetic(case):
    from dedark_yolo_amd.nn.tasks import TTA, tta_plan
    (H, W, strides), sizes, counts, tail, head, total = case
    passes, a_total = tta_plan(H, W, strides, len(strides))
    assert a_total == total
    assert [(p[4], p[5]) for p in passes] == sizes
    assert [p[6] for p in passes] == counts
    assert [(p[0], p[1]) for p in passes] == list(zip(TTA["scales"], TTA["flips"])) == [(1, None), (0.83, 3), (0.67, None)]
    # resized sizes: Python int() of the double product; the first pass is the image itself
    assert [(p[2], p[3]) for p in passes] == [(H, W), (int(H * 0.83), int(W * 0.83)), (int(H * 0.67), int(W * 0.67))]
    (_, _, _, _, _, _, A0, lo0, hi0, c0), (_, _, _, _, _, _, A1, lo1, hi1, c1), (_, _, _, _, _, _, A2, lo2, hi2, c2) = passes
    assert (lo0, A0 - hi0) == (0, tail) and (lo1, hi1) == (0, A1) and (lo2, hi2) == (head, A2)
    assert (c0, c1, c2) == (0, hi0, hi0 + A1) and c2 + (hi2 - lo2) == total


def test_tta_plan_matches_level_extents_on_stride_multiples():
    """For sizes that are multiples of the largest stride the integer formula is 'the coarsest level of pass 0, the finest level
    of the last pass'."""
    from dedark_yolo_amd.nn.tasks import tta_plan
    for H, W, strides in ((128, 128, (8, 16, 32)), (256, 192, (8, 16, 32, 64)), (128, 128, (4, 8, 16, 32))):
        passes, _ = tta_plan(H, W, strides, len(strides))
        Hp, Wp = passes[0][4:6]
        assert passes[0][6] - passes[0][8] == (Hp // strides[-1]) * (Wp // strides[-1])
        Hp, Wp = passes[2][4:6]
        assert passes[2][7] == (Hp // strides[0]) * (Wp // strides[0])
    with pytest.raises(ValueError):
        tta_plan(128, 128, (8, 16, 32), 4)


def test_cfg_has_the_augment_key():
    from dedark_yolo_amd.engine.trainer import get_cfg
    assert get_cfg().augment is False
    assert get_cfg(dict(augment=True)).augment is True


def test_c_abi_declares_the_tta_entries():
    from dedark_yolo_amd import _C
    with open(os.path.join(ROOT, "include", "dedark_yolo.h")) as f:
        header = f.read()
    for name, nargs in (("dy_tta_scale_img", 12), ("dy_detect_decode_tta", 11)):
        assert name in _C._SIGS and name in _C.exported_symbols()
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared in include/dedark_yolo.h"
        assert len(m.group(1).split(",")) == nargs == len(_C._SIGS[name])
    with open(os.path.join(ROOT, "dedark_yolo_amd", "csrc", "Makefile")) as f:
        assert "tta.hip" in f.read()


def _tiny_detect():
    from dedark_yolo_amd.nn.tasks import DetectionModel
    cfg = load_yaml("yolov8ori.yaml")
    cfg["scales"]["t"] = [0.33, 0.125, 1024]
    cfg["scale"] = "t"
    return DetectionModel(cfg, nc=20)


def test_augment_rejects_a_batch_dict_and_training_mode_does_not_augment():
    model = _tiny_detect()
    with pytest.raises(ValueError, match="image tensor"):
        model.predict(dict(img=torch.zeros(1, 3, 64, 64)), augment=True)
    model.eval()
    with pytest.raises(ValueError, match="multiple"):           # _check_imgsz guards the augmented path too
        model.predict(torch.zeros(1, 3, 72, 64), augment=True)
    called = []
    model._predict_augment = lambda x: called.append("augment")
    model._predict_once = lambda x, *a, **k: called.append("once")
    model.train()
    model.predict(torch.zeros(1, 3, 64, 64), augment=True)
    model.eval()
    model.predict(torch.zeros(1, 3, 64, 64), augment=True)
    model.predict(torch.zeros(1, 3, 64, 64))
    assert called == ["once", "augment", "once"]


def test_only_the_detection_model_augments():
    """reference tasks.py:121-127, 358-363, 381-386: the base, segment and pose models warn and run single-scale."""
    from dedark_yolo_amd.nn.tasks import BaseModel, ClassificationModel, DetectionModel, PoseModel, SegmentationModel
    assert DetectionModel._predict_augment is not BaseModel._predict_augment
    for cls in (SegmentationModel, PoseModel, ClassificationModel):
        assert cls._predict_augment is BaseModel._predict_augment

    class Probe(BaseModel):
        def _predict_once(self, x, profile=False, visualize=False):
            return "single"
    with pytest.warns(UserWarning, match="single-scale"):
        assert Probe().eval().predict(torch.zeros(1), augment=True) == "single"

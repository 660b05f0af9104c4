"""Segment inference at image resolution, the parts that need no GPU: the two kernels are declared in the header and bound, the
scale_masks window arithmetic equals what the reference computed (tests/golden/make_segpredict_golden.py), the `Masks` /
`Results(masks=...)` surface, and the two cfg keys."""
import os
import re

import pytest
import torch

from util import gold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kernels_are_declared_and_bound():
    from dedark_yolo_amd import _C
    with open(os.path.join(ROOT, "include", "dedark_yolo.h")) as f:
        header = f.read()
    for name in ("dy_seg_mask_upsample", "dy_mask_resize"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/dedark_yolo.h"
        assert name in _C._SIGS and name in _C.exported_symbols()
        assert len(_C._SIGS[name]) == len(m.group(1).split(",")), f"{name}: binding and prototype disagree on the argument count"


def test_scale_masks_window_equals_the_reference():
    from dedark_yolo_amd.utils.ops import scale_masks_window
    g = gold("g18_maskup")
    for tag in ("n0", "n1", "n2"):
        shape = tuple(int(v) for v in g[tag + "_shape"])
        assert scale_masks_window(40, 40, shape) == tuple(int(v) for v in g[tag + "_window"]), tag
    g = gold("g18_scalemasks")
    seen = set()
    for si in (0, 1):
        for padding in (True, False):
            k = f"sm{si}_{int(padding)}"
            shape = tuple(int(v) for v in g[k + "_shape"])
            win = scale_masks_window(40, 40, shape, padding)
            assert win == tuple(int(v) for v in g[k + "_window"]), k
            seen.add(win)
    assert len(seen) == 4 and any(w[0] > 0 for w in seen) and any(w[1] > 0 for w in seen)       # vertical and horizontal crops both occur


def test_masks_and_results_surface():
    from dedark_yolo_amd.engine.results import Masks, Results
    data = (torch.arange(3 * 4 * 5).view(3, 4, 5) % 2).float()
    m = Masks(data, (40, 50))
    assert len(m) == 3 and tuple(m.shape) == (3, 4, 5) and m.orig_shape == (40, 50) and m.data is data
    c = m.cpu()
    assert isinstance(c, Masks) and torch.equal(c.data, data) and c.orig_shape == (40, 50)
    one = Masks(data[0], (40, 50))
    assert tuple(one.data.shape) == (1, 4, 5) and len(one) == 1
    for attr in ("xy", "xyn"):
        with pytest.raises(NotImplementedError, match="findContours"):
            getattr(m, attr)
    boxes = torch.zeros(3, 6)
    r = Results((40, 50), boxes, masks=data)
    assert isinstance(r.masks, Masks) and len(r.masks) == 3 and r.masks.orig_shape == (40, 50) and len(r) == 3
    assert Results((40, 50), boxes).masks is None
    assert Results((40, 50), boxes[:0], masks=None).masks is None


def test_default_cfg_has_the_segment_inference_keys():
    from dedark_yolo_amd.engine.trainer import get_cfg
    a = get_cfg()
    assert a.retina_masks is False and a.save_json is False


def test_batched_mode_names_are_checked_before_any_device_work():
    from dedark_yolo_amd.utils import ops as uops
    assert uops.MASK_MODES == ("proto", "input", "upsample", "native")
    with pytest.raises(ValueError):
        uops.process_masks_batched(torch.zeros(1, 32, 4, 4), [torch.zeros(0, 38)], (16, 16), mode="bilinear")

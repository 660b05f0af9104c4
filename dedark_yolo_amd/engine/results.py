"""Minimal prediction containers with the attribute surface of the reference's ultralytics/engine/results.py:
`Results.boxes` -> `Boxes` with `.data` ([n,6] xyxy, conf, cls), `.xyxy`, `.conf`, `.cls`, `.xywh`, `.xyxyn`, `len()`; `Results`
also carries `orig_shape`, `names`, for a pose model `keypoints` -> `Keypoints` (`.data`, `.xy`, `.xyn`, `.conf`) and for a segment
model `masks` -> `Masks` (`.data`).  Plotting / saving helpers and the mask contours (`Masks.xy` / `.xyn`) are outside the hot path."""
import torch

from ..utils import ops


class Boxes:
    def __init__(self, data, orig_shape):
        if data.ndim == 1:
            data = data[None, :]
        assert data.shape[-1] == 6, "Boxes expects rows of (x1, y1, x2, y2, conf, cls)"
        self.data = data
        self.orig_shape = orig_shape

    @property
    def xyxy(self):
        return self.data[:, :4]

    @property
    def conf(self):
        return self.data[:, 4]

    @property
    def cls(self):
        return self.data[:, 5]

    @property
    def xywh(self):
        return ops.xyxy2xywh(self.xyxy)

    @property
    def xyxyn(self):
        h, w = self.orig_shape
        return self.xyxy / torch.tensor([w, h, w, h], dtype=self.data.dtype, device=self.data.device)

    def cpu(self):
        return Boxes(self.data.cpu(), self.orig_shape)

    def __len__(self):
        return self.data.shape[0]


class Keypoints:
    """reference engine/results.py:521-566: data [n, K, 2 or 3] (pixels of orig_shape, plus the visibility score for ndim 3),
    `.xy`, `.xyn` (normalised by orig_shape), `.conf` (None for ndim 2), `.has_visible`."""

    def __init__(self, keypoints, orig_shape):
        if keypoints.ndim == 2:
            keypoints = keypoints[None, :]
        self.data = keypoints
        self.orig_shape = tuple(orig_shape)
        self.has_visible = self.data.shape[-1] == 3

    @property
    def xy(self):
        return self.data[..., :2]

    @property
    def xyn(self):
        xy = self.xy.clone()
        xy[..., 0] /= self.orig_shape[1]
        xy[..., 1] /= self.orig_shape[0]
        return xy

    @property
    def conf(self):
        return self.data[..., 2] if self.has_visible else None

    def cpu(self):
        return Keypoints(self.data.cpu(), self.orig_shape)

    def __len__(self):
        return self.data.shape[0]


class Masks:
    """reference engine/results.py:464-518: data [n, h, w] of 0 / 1 (f32, as process_mask returns it), `orig_shape`, `len()`,
    `.cpu()`; a single [h, w] mask gains the leading axis.  `.xy` / `.xyn` (the reference's masks2segments contours) need
    cv2.findContours and are not implemented."""

    def __init__(self, masks, orig_shape):
        if masks.ndim == 2:
            masks = masks[None, :]
        self.data = masks
        self.orig_shape = tuple(orig_shape)

    @property
    def shape(self):
        return self.data.shape

    @property
    def xy(self):
        raise NotImplementedError("Masks.xy: mask contours need cv2.findContours (masks2segments), which is outside the hot path")

    @property
    def xyn(self):
        raise NotImplementedError("Masks.xyn: mask contours need cv2.findContours (masks2segments), which is outside the hot path")

    def cpu(self):
        return Masks(self.data.cpu(), self.orig_shape)

    def __len__(self):
        return self.data.shape[0]


class Results:
    def __init__(self, orig_shape, boxes, names=None, path=None, keypoints=None, masks=None):
        self.orig_shape = tuple(orig_shape)
        self.boxes = Boxes(boxes, self.orig_shape)
        self.keypoints = Keypoints(keypoints, self.orig_shape) if keypoints is not None else None
        self.masks = Masks(masks, self.orig_shape) if masks is not None else None
        self.names = names
        self.path = path

    def __len__(self):
        return len(self.boxes)

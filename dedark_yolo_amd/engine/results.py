"""Minimal prediction containers with the attribute surface of the reference's ultralytics/engine/results.py:
`Results.boxes` -> `Boxes` with `.data` ([n,6] xyxy, conf, cls), `.xyxy`, `.conf`, `.cls`, `.xywh`, `.xyxyn`, `len()`; `Results`
also carries `orig_shape`, `names` and, for a pose model, `keypoints` -> `Keypoints` (`.data`, `.xy`, `.xyn`, `.conf`).  Plotting / saving helpers are outside the hot path."""
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


class Results:
    def __init__(self, orig_shape, boxes, names=None, path=None, keypoints=None):
        self.orig_shape = tuple(orig_shape)
        self.boxes = Boxes(boxes, self.orig_shape)
        self.keypoints = Keypoints(keypoints, self.orig_shape) if keypoints is not None else None
        self.names = names
        self.path = path

    def __len__(self):
        return len(self.boxes)

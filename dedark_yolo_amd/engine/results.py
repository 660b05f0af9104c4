"""Minimal prediction containers with the attribute surface of the reference's ultralytics/engine/results.py:
`Results.boxes` -> `Boxes` with `.data` ([n,6] xyxy, conf, cls), `.xyxy`, `.conf`, `.cls`, `.xywh`, `.xyxyn`, `len()`; `Results`
also carries `orig_shape`, `names`, for a pose model `keypoints` -> `Keypoints` (`.data`, `.xy`, `.xyn`, `.conf`) and for a segment
model `masks` -> `Masks` (`.data`); a classify model fills `probs` -> `Probs` (`.data`, `.top1`, `.top5`, `.top1conf`, `.top5conf`)
and leaves `boxes` None.  Plotting / saving helpers and the mask contours (`Masks.xy` / `.xyn`) are outside the hot path."""
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


class Probs:
    """reference engine/results.py:569-615: data [nc] class probabilities of one image, `.top1` (int), `.top5` (list of the
    min(nc, 5) best indices, descending), `.top1conf`, `.top5conf` (tensors).  On the device the indices come from dy_cls_topk,
    on the host from a stable descending sort: equal probabilities rank by ascending index either way."""

    def __init__(self, probs, orig_shape=None):
        self.data = probs
        self.orig_shape = orig_shape

    @property
    def top5(self):
        c = self.__dict__.get("_top5")
        if c is None:
            d = self.data
            if d.is_cuda:
                from .. import ops as kops
                c = kops.cls_topk(d.reshape(1, -1))[0].tolist()
            else:
                c = torch.sort(d.float(), descending=True, stable=True).indices[:min(d.numel(), 5)].tolist()
            self.__dict__["_top5"] = c
        return c

    @property
    def top1(self):
        return int(self.top5[0])

    @property
    def top1conf(self):
        return self.data[self.top1]

    @property
    def top5conf(self):
        return self.data[self.top5]

    def cpu(self):
        return Probs(self.data.cpu(), self.orig_shape)

    def __len__(self):
        return self.data.shape[0]


class Results:
    def __init__(self, orig_shape, boxes=None, names=None, path=None, keypoints=None, masks=None, probs=None):
        self.orig_shape = tuple(orig_shape)
        self.boxes = Boxes(boxes, self.orig_shape) if boxes is not None else None
        self.probs = Probs(probs, self.orig_shape) if probs is not None else None
        self.keypoints = Keypoints(keypoints, self.orig_shape) if keypoints is not None else None
        self.masks = Masks(masks, self.orig_shape) if masks is not None else None
        self.names = names
        self.path = path

    def __len__(self):
        """The first of boxes / masks / probs / keypoints that is set (reference results.py:152-164): the class count for a
        classify result."""
        for v in (self.boxes, self.masks, self.probs, self.keypoints):
            if v is not None:
                return len(v)
        return 0

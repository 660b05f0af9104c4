"""Detect-task validator with the reference's structure (ultralytics/engine/validator.py:95-200 `__call__` loop,
ultralytics/models/yolo/detect/val.py:30-174): preprocess -> model (eval) -> batched HIP NMS -> per-image greedy matching at
10 IoU thresholds -> AP per class / mAP50 / mAP50-95 / fitness.

The device part (img/255, front-end, network, Detect decode, NMS) stays on the GPU; one D2H copy per batch brings the kept
detections to the host, where the matching and AP bookkeeping run in numpy exactly as in the reference (val.py:151-174 uses
numpy for the matching as well)."""
import numpy as np
import torch

from .. import ops as kops
from .._C import call
from ..ops import ptr, stream
from ..utils import ops
from ..utils.metrics import ClassifyMetrics, DetMetrics, PoseMetrics, SegmentMetrics, box_iou, kpt_iou, oks_sigmas


def match_predictions(detections, labels, iouv):
    """Which detections count as true positives at each IoU threshold: detections [N,6] (xyxy, conf, cls), labels [M,5] (cls, xyxy),
    host tensors -> bool [N, len(iouv)].  The rule of the reference's `_process_batch` (ultralytics/models/yolo/detect/val.py:151-174),
    stated directly instead of through its sort / unique calls: per threshold, among the (label, detection) pairs of equal class with
    IoU >= threshold,
      1. every detection keeps ONE label, the one it overlaps most (an exact IoU tie goes to the higher label index: the order the
         reference's reversed ascending sort leaves equal keys in);
      2. every label keeps ONE of the detections that chose it -- the one with the LOWEST detection index (its second `np.unique` runs on
         rows that the first one has re-ordered by detection index, so it is not the best-overlapping one).
    The detections that survive both steps are correct at that threshold."""
    iou = box_iou(labels[:, 1:], detections[:, :4]).numpy()
    return match_from_iou(iou, labels[:, 0], detections[:, 5], iouv)


def match_from_iou(iou, label_cls, det_cls, iouv):
    """match_predictions' rule on a precomputed IoU matrix [n_labels, n_detections] (numpy; the mask IoU of the segment validator,
    reference segment/val.py:185-209): label_cls [M], det_cls [N] host tensors -> bool [N, len(iouv)]."""
    n_lab, n_det = iou.shape
    correct = np.zeros((n_det, len(iouv)), dtype=bool)
    if n_lab == 0 or n_det == 0:
        return torch.from_numpy(correct)
    same_cls = (label_cls.view(-1, 1) == det_cls.view(1, -1)).numpy()
    thr = np.asarray(iouv, dtype=iou.dtype)
    for k in range(len(thr)):
        cand = (iou >= thr[k]) & same_cls
        dets = np.flatnonzero(cand.any(0))
        if dets.size == 0:
            continue
        score = np.where(cand[:, dets], iou[:, dets], -1.0)
        chosen = n_lab - 1 - np.argmax(score[::-1], axis=0)          # step 1 (argmax of the flipped column: last maximum)
        keep = np.unique(chosen, return_index=True)[1]               # step 2: first = lowest detection index per label
        correct[dets[keep], k] = True
    return torch.from_numpy(correct)


class DetectionValidator:
    n_task = 0          # `correct` matrices per image besides the box one (_task_correct)

    def __init__(self, args=None, dataloader=None):
        from .trainer import get_cfg
        self.args = args if args is not None else get_cfg()
        self.dataloader = dataloader
        self.iouv = torch.linspace(0.5, 0.95, 10)
        self.niou = self.iouv.numel()
        self.metrics = DetMetrics()
        self.device = None
        self.training = False
        # engine/validator.py:86-87: conf None -> 0.001; this fork's default.yaml:48 sets conf 0.25, which therefore applies
        self.conf = 0.001 if getattr(self.args, "conf", None) is None else self.args.conf

    # ------------------------------------------------------------------------------------------ per batch
    def preprocess(self, batch):
        """val.py:30-41: uint8 -> float / 255 on the device (no darkening at validation time)."""
        img = batch["img"]
        if img.dtype != torch.uint8:
            raise RuntimeError("validator expects the dataloader's uint8 image tensor")
        img = img.to(self.device, non_blocking=True).contiguous()
        out = torch.empty(img.shape, dtype=torch.float32, device=self.device)
        acc = torch.zeros(1, dtype=torch.float64, device=self.device)
        call("dy_preprocess_batch", ptr(img), ptr(out), None, 1.0, 0, 0, ptr(acc), img.numel(), stream())
        batch["img"] = out
        return batch

    def postprocess(self, preds, nc=0):
        """NMS on the eval output; `nc` = the class count when task columns follow the class scores (segment, pose)."""
        a = self.args
        return ops.non_max_suppression(preds, self.conf, a.iou, multi_label=True, agnostic=bool(getattr(a, "single_cls", False)),
                                       max_det=a.max_det, nc=nc)

    def init_metrics(self, model):
        self.nc = model.model[-1].nc
        self.names = getattr(model, "names", None) or {i: str(i) for i in range(self.nc)}
        self.metrics.names = self.names
        self.seen = 0
        self.stats = []

    def update_metrics(self, preds, batch):
        """val.py:72-116 on host copies.  Per image one row of `self.stats`: the box `correct` matrix, the task's own ones
        (`_task_correct`; `n_task` of them), confidences, predicted classes, label classes."""
        bi = batch["batch_idx"].cpu()
        cls_all, box_all = batch["cls"].cpu().float(), batch["bboxes"].cpu().float()
        height, width = batch["img"].shape[2:]
        for si, pred in enumerate(preds):
            pred = pred.cpu()
            idx = bi == si
            cls, bbox = cls_all[idx], box_all[idx]
            nl, npr = cls.shape[0], pred.shape[0]
            shape = batch["ori_shape"][si] if "ori_shape" in batch else (height, width)
            ratio_pad = batch["ratio_pad"][si] if "ratio_pad" in batch else None
            correct = [torch.zeros(npr, self.niou, dtype=torch.bool) for _ in range(1 + self.n_task)]
            self.seen += 1
            if npr == 0:
                if nl:
                    self.stats.append((*correct, torch.zeros(0), torch.zeros(0), cls.squeeze(-1)))
                continue
            if getattr(self.args, "single_cls", False):
                pred[:, 5] = 0
            predn = pred.clone()
            ops.scale_boxes((height, width), predn[:, :4], shape, ratio_pad=ratio_pad)
            if nl:
                tbox = ops.xywh2xyxy(bbox) * torch.tensor((width, height, width, height), dtype=torch.float32)
                ops.scale_boxes((height, width), tbox, shape, ratio_pad=ratio_pad)
                labelsn = torch.cat((cls, tbox), 1)
                correct = [match_predictions(predn, labelsn, self.iouv),
                           *self._task_correct(batch, si, idx, predn, labelsn, shape, ratio_pad)]
            self.stats.append((*correct, pred[:, 4], pred[:, 5], cls.squeeze(-1)))

    def _task_correct(self, batch, si, idx, predn, labelsn, shape, ratio_pad):
        """The task's own `correct` matrices of image `si` (labels `idx` of the batch; predn / labelsn scaled to `shape`)."""
        return ()

    def get_stats(self):
        """val.py:123-129"""
        if not self.stats:
            self.nt_per_class = np.zeros(self.nc, dtype=int)
            return self.metrics.results_dict
        stats = [torch.cat(x, 0).numpy() for x in zip(*self.stats)]
        if len(stats) and stats[0].any():
            self.metrics.process(*stats)
        self.nt_per_class = np.bincount(stats[-1].astype(int), minlength=self.nc)
        return self.metrics.results_dict

    # ------------------------------------------------------------------------------------------ loop
    @torch.no_grad()
    def __call__(self, model, dataloader=None, dtype=None):
        """engine/validator.py:95-200 (model given directly; the trainer passes its EMA weights loaded into `model`)."""
        loader = dataloader if dataloader is not None else self.dataloader
        if loader is None:
            raise ValueError("pass an iterable of reference-schema batch dicts (YOLO.val(data=<data yaml>) builds one from a dataset on disk)")
        self.device = next(model.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError("DetectionValidator needs the model on a GPU (there is no CPU path)")
        if dtype is not None:
            kops.set_compute_dtype(dtype)
        was_training = model.training
        model.eval()
        self.init_metrics(model)
        for batch in loader:
            batch = self.preprocess(dict(batch))
            # engine/validator.py:99,170: augmented inference only outside the trainer's own validation
            preds = model(batch["img"], augment=bool(getattr(self.args, "augment", False)) and not self.training)
            preds = self.postprocess(preds)
            self.update_metrics(preds, batch)
        stats = self.get_stats()
        model.train(was_training)
        return {k: float(v) for k, v in stats.items()}


class SegmentationValidator(DetectionValidator):
    """Segment validator (reference models/yolo/segment/val.py): NMS with the mask-coefficient columns, predicted masks of the whole
    batch in one launch, mask IoU against the gt masks with integer counts (dy_seg_mask_iou), box and mask `correct` matrices by
    the same matching rule, SegmentMetrics.  `process` as in init_metrics (val.py:31-39): save_json False -> process_mask at the
    proto resolution (dy_seg_mask_decode), save_json True -> process_mask_upsample at the input resolution
    (dy_seg_mask_upsample).  gt masks (index maps or planes) at another resolution than the predicted masks are resized
    bilinearly and thresholded at 0.5 (val.py:146-148; dy_mask_resize).  Writing predictions.json itself (RLE through pycocotools,
    scale_image through cv2) is out of scope: save_json only selects the masks that are evaluated."""

    n_task = 1

    def __init__(self, args=None, dataloader=None):
        super().__init__(args, dataloader)
        self.args.task = "segment"
        self.metrics = SegmentMetrics()

    def postprocess(self, preds):
        proto = preds[1][-1] if len(preds[1]) == 3 else preds[1]
        return super().postprocess(preds[0], nc=self.nc), proto

    def update_metrics(self, preds, batch):
        dets, proto = preds
        height, width = batch["img"].shape[2:]
        mode = "upsample" if getattr(self.args, "save_json", False) else "proto"
        pmasks = ops.process_masks_batched(proto, [d[:, :6 + proto.shape[1]] for d in dets], (height, width), mode=mode)
        super().update_metrics(dets, dict(batch, masks=batch["masks"].to(self.device, non_blocking=True), pmasks=pmasks))

    def _task_correct(self, batch, si, idx, predn, labelsn, shape, ratio_pad):
        overlap, masks = bool(getattr(self.args, "overlap_mask", True)), batch["masks"]
        gt = masks[si] if overlap else masks[idx.to(masks.device)]
        pred, m = batch["pmasks"][si], labelsn.shape[0]
        if tuple(gt.shape[-2:]) != tuple(pred.shape[-2:]) and m:
            gt = ops.resize_masks(gt, pred.shape[-2:], m=m if overlap else None)       # -> uint8 planes [m, h, w]
            overlap = False
        iou_m = ops.mask_iou_binary(gt, pred, overlap, m).cpu().numpy()
        return (match_from_iou(iou_m, labelsn[:, 0], predn[:, 5], self.iouv),)


class PoseValidator(DetectionValidator):
    """Pose validator (reference models/yolo/pose/val.py): NMS with multi_label and the K * ndim keypoint columns appended,
    boxes (scale_boxes) and keypoints (scale_coords) to ori_shape / ratio_pad, OKS against the gt keypoints in native space with
    area = gt box w * h * 0.53 (kpt_iou on dy_kpt_oks), box and pose `correct` matrices by the same matching rule, PoseMetrics.
    sigma = metrics.oks_sigmas(kpt_shape)."""

    n_task = 1

    def __init__(self, args=None, dataloader=None):
        super().__init__(args, dataloader)
        self.args.task = "pose"
        self.metrics = PoseMetrics()

    def init_metrics(self, model):
        super().init_metrics(model)
        self.kpt_shape = list(model.model[-1].kpt_shape)
        self.sigma = oks_sigmas(self.kpt_shape)

    def postprocess(self, preds):
        return super().postprocess(preds, nc=self.nc)

    def update_metrics(self, preds, batch):
        """val.py:62-109 on host copies (the OKS matrix on the device)."""
        if "keypoints" not in batch:
            raise ValueError("pose validation: the batch has no 'keypoints'")
        super().update_metrics(preds, dict(batch, keypoints=batch["keypoints"].cpu().float()))

    def _task_correct(self, batch, si, idx, predn, labelsn, shape, ratio_pad):
        height, width = batch["img"].shape[2:]
        kpts = batch["keypoints"][idx]
        nk = kpts.shape[1] if kpts.dim() == 3 else int(self.kpt_shape[0])
        pred_kpts = predn[:, 6:].view(predn.shape[0], nk, -1)
        ops.scale_coords((height, width), pred_kpts, shape, ratio_pad=ratio_pad)
        tkpts = kpts.clone()
        tkpts[..., 0] *= width
        tkpts[..., 1] *= height
        tkpts = ops.scale_coords((height, width), tkpts, shape, ratio_pad=ratio_pad)
        area = ops.xyxy2xywh(labelsn[:, 1:])[:, 2:].prod(1) * 0.53
        oks = kpt_iou(tkpts.to(self.device), pred_kpts.to(self.device), area, self.sigma).cpu().numpy()
        return (match_from_iou(oks, labelsn[:, 0], predn[:, 5], self.iouv),)


class ClassificationValidator:
    """Classify validator (reference models/yolo/classify/val.py:39-60, engine/validator.py:95-200): preprocess -> eval forward
    (soft-max probabilities) -> dy_cls_topk (k = min(nc, 5)) -> dy_cls_metrics_update.  The hit counts and the confusion matrix
    ([pred top-1][target], ConfusionMatrix.process_cls_preds, metrics.py:197-207) stay on the device: nothing is read back per
    batch, `get_stats` reads both once.  A batch is {img: uint8 or float [B, 3, H, W], cls: int64 [B]}; there is no
    validation-loss column and no plotting."""

    def __init__(self, args=None, dataloader=None):
        from .trainer import get_cfg
        self.args = args if args is not None else get_cfg()
        self.args.task = "classify"
        self.dataloader = dataloader
        self.metrics = ClassifyMetrics()
        self.device = None
        self.training = False
        self.confusion_matrix = None
        self._acc = None

    def preprocess(self, batch):
        """val.py:32-37: img to the device as float, cls to the device; a uint8 image additionally becomes f32 / 255 on the device."""
        from ..utils.loss import classify_batch_to_device
        if self._acc is None or self._acc.device != self.device:
            self._acc = torch.zeros(1, dtype=torch.float64, device=self.device)
        return classify_batch_to_device(batch, self.device, self._acc)

    def init_metrics(self, model):
        self.nc = len(model.names) if getattr(model, "names", None) else int(model.yaml["nc"])
        self.names = getattr(model, "names", None) or {i: str(i) for i in range(self.nc)}
        self.metrics.names = self.names
        self.counts = torch.zeros(3, dtype=torch.int64, device=self.device)
        self._confusion = torch.zeros((self.nc, self.nc), dtype=torch.int32, device=self.device)
        self.confusion_matrix = None

    def update_metrics(self, preds, batch):
        """val.py:39-43 on the device: the k best classes per row, then the counters."""
        preds = preds[0] if isinstance(preds, (list, tuple)) else preds
        idx = kops.cls_topk(preds)
        kops.cls_metrics_update(idx, batch["cls"], self.nc, self.counts, self._confusion)

    def get_stats(self):
        """val.py:45-60 (finalize_metrics, get_stats): the one read-back of the run."""
        self.metrics.process_counts(self.counts.cpu().tolist())
        self.confusion_matrix = self._confusion.cpu().numpy().astype(np.int64)
        return self.metrics.results_dict

    @torch.no_grad()
    def __call__(self, model, dataloader=None, dtype=None):
        loader = dataloader if dataloader is not None else self.dataloader
        if loader is None:
            raise ValueError("pass an iterable of {img, cls} batch dicts; dataset decoding is outside the hot path")
        self.device = next(model.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError("ClassificationValidator needs the model on a GPU (there is no CPU path)")
        if dtype is not None:
            kops.set_compute_dtype(dtype)
        was_training = model.training
        model.eval()
        self.init_metrics(model)
        for batch in loader:
            batch = self.preprocess(dict(batch))
            self.update_metrics(model(batch["img"], augment=bool(getattr(self.args, "augment", False)) and not self.training), batch)
        stats = self.get_stats()
        model.train(was_training)
        return {k: float(v) for k, v in stats.items()}

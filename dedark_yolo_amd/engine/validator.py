"""Detect-task validator with the reference's structure (ultralytics/engine/validator.py:95-200 `__call__` loop,
ultralytics/models/yolo/detect/val.py:30-174): preprocess -> model (eval) -> batched HIP NMS -> per-image greedy matching at
10 IoU thresholds -> AP per class / mAP50 / mAP50-95 / fitness.

The device part (img/255, front-end, network, Detect decode, NMS, box scaling, IoU, matching, confusion matrix: csrc/nms.hip,
csrc/valmatch.hip) stays on the GPU; the detect batch loop copies nothing to the host.  `get_stats` reads the matched-prediction
table and the confusion matrix back once, and the AP bookkeeping runs in numpy as in the reference."""
import json
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

from .. import ops as kops
from .._C import call
from ..ops import ptr, stream
from ..utils import ops
from ..utils.metrics import LOGGER, ClassifyMetrics, ConfusionMatrix, DetMetrics, PoseMetrics, SegmentMetrics, box_iou, kpt_iou, oks_sigmas


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


def scale_record(img1_shape, img0_shape, ratio_pad=None):
    """(gain, pad_x, pad_y, h0, w0) of one image exactly as utils/ops.scale_boxes derives them (ops.py:44-56): with `ratio_pad`
    its ratio_pad[0][0] and ratio_pad[1], else the min / round(... - 0.1) rule.  dy_val_box_match reads the five as f32."""
    if ratio_pad is None:
        gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
        pad = round((img1_shape[1] - img0_shape[1] * gain) / 2 - 0.1), round((img1_shape[0] - img0_shape[0] * gain) / 2 - 0.1)
    else:
        gain = ratio_pad[0][0]
        pad = ratio_pad[1]
    return [float(gain), float(pad[0]), float(pad[1]), float(img0_shape[0]), float(img0_shape[1])]


def save_one_txt(predn, save_conf, shape, file):
    """detect/val.py:212-219: one `cls x y w h [conf]` line per row of predn [n, 6] (native-space xyxy, conf, cls; host), the box
    normalised by the original (h, w) `shape`, every number through %g."""
    gn = torch.tensor(shape)[[1, 0, 1, 0]]
    xywh = (ops.xyxy2xywh(predn[:, :4].float()) / gn).tolist()
    lines = []
    for (*_, conf, cls), box in zip(predn.tolist(), xywh):
        line = (cls, *box, conf) if save_conf else (cls, *box)
        lines.append(("%g " * len(line)).rstrip() % line + "\n")
    with open(file, "w") as f:
        f.writelines(lines)


def pred_to_json(predn, filename):
    """detect/val.py:221-232: the COCO-style records of predn [n, 6] (host): image_id = the integer stem when it is numeric, bbox =
    top-left xywh rounded to 3 places, score rounded to 5, category_id = the class."""
    stem = Path(filename).stem
    image_id = int(stem) if stem.isnumeric() else stem
    box = ops.xyxy2xywh(predn[:, :4].float())
    box[:, :2] -= box[:, 2:] / 2
    return [dict(image_id=image_id, category_id=int(p[5]), bbox=[round(x, 3) for x in b], score=round(p[4], 5))
            for p, b in zip(predn.tolist(), box.tolist())]


class DetectionValidator:
    """Detect validator.  Per batch: batched NMS (`postprocess` keeps its padded [B, max_det, 6] rows and counts on the device), then ONE
    dy_val_box_match launch for the whole batch: native-space boxes, the `correct` matrix at the 10 IoU thresholds and the confusion
    matrix.  Nothing is copied to the host inside the batch loop; `get_stats` (or the first read of `.stats`) reads everything back
    once.  `match_predictions` / `match_from_iou` above stay as the host statement of the rule the kernel applies."""

    n_task = 0          # `correct` matrices per image besides the box one (_task_iou)

    def __init__(self, args=None, dataloader=None, save_dir=None):
        from .trainer import get_cfg
        self.args = args if args is not None else get_cfg()
        self.dataloader = dataloader
        self.iouv = torch.linspace(0.5, 0.95, 10)
        self.niou = self.iouv.numel()
        self.metrics = DetMetrics()
        self.device = None
        self.training = False
        a = self.args
        save_dir = save_dir if save_dir is not None else getattr(a, "save_dir", None)
        if save_dir is None and (getattr(a, "project", None) or getattr(a, "name", None)):
            save_dir = Path(a.project or "runs") / (a.name or "val")
        self.save_dir = None if save_dir is None else Path(save_dir)
        self.confusion_matrix = None
        self.nt_per_class = None
        self.jdict = []
        # engine/validator.py:86-87: conf None -> 0.001; this fork's default.yaml:48 sets conf 0.25, which therefore applies
        self.conf = 0.001 if getattr(self.args, "conf", None) is None else self.args.conf

    def _flag(self, name, default=False):
        return bool(getattr(self.args, name, default))

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
        """NMS on the eval output.  Detect (nc == 0): the padded rows [B, max_det, 6] and the counts [B] as nms_batched leaves them,
        both on the device.  `nc` = the class count when task columns follow the class scores (segment, pose): the per-image list of
        non_max_suppression, whose counts those validators need on the host anyway."""
        a = self.args
        if nc:
            return ops.non_max_suppression(preds, self.conf, a.iou, multi_label=True, agnostic=self._flag("single_cls"), max_det=a.max_det,
                                           nc=nc)
        if isinstance(preds, (list, tuple)):
            preds = preds[0]
        return ops.nms_batched(preds, self.conf, a.iou, True, self._flag("single_cls"), a.max_det, 30000, 7680)

    def init_metrics(self, model):
        self.nc = model.model[-1].nc
        self.names = getattr(model, "names", None) or {i: str(i) for i in range(self.nc)}
        self.metrics.names = self.names
        self.seen = 0
        self.stats = []
        self.jdict = []
        self.confusion_matrix = ConfusionMatrix(nc=self.nc)
        self._confusion = torch.zeros((self.nc + 1, self.nc + 1), dtype=torch.int32, device=self.device)
        self._iouv_dev = self.iouv.to(self.device)

    # `stats`: one row per image that has predictions or labels -- (correct matrices ..., conf, predicted cls, label cls), host tensors.
    # update_metrics only queues device tensors; the rows are built, with one read-back for everything queued, when they are first read.
    @property
    def stats(self):
        if self._pending:
            self._rows.extend(self._read_back(self._pending))
            self._pending = []
        return self._rows

    @stats.setter
    def stats(self, rows):
        self._rows, self._pending = list(rows), []

    def _read_back(self, pending):
        def host(parts):
            dev = [p for p in parts if p.is_cuda]                 # one copy for all of them
            if dev:
                flat = iter(torch.cat([p.reshape(-1) for p in dev]).cpu().split([p.numel() for p in dev]))
                parts = [next(flat).view(p.shape) if p.is_cuda else p for p in parts]
            return parts
        n_cor = 1 + self.n_task
        cors = [host([q["correct"][k] for q in pending]) for k in range(n_cor)]
        ccs = host([q["cc"] for q in pending])
        cnts = [q["lens"] for q in pending]
        if any(c is None for c in cnts):
            got = iter(host([q["cnt"] for q in pending if q["lens"] is None]))
            cnts = [c if c is not None else next(got).tolist() for c in cnts]
        tcls = host([q["tcls"] for q in pending])
        loffs = [q["loff_h"] for q in pending]
        if any(l is None for l in loffs):
            got = iter(host([q["loff"] for q in pending if q["loff_h"] is None]))
            loffs = [l if l is not None else next(got).tolist() for l in loffs]
        rows = []
        for i in range(len(pending)):
            for b, n in enumerate(cnts[i]):
                l0, l1 = loffs[i][b], loffs[i][b + 1]
                if n == 0 and l1 == l0:
                    continue
                rows.append((*(cors[k][i][b, :n].bool() for k in range(n_cor)), ccs[i][b, :n, 0], ccs[i][b, :n, 1], tcls[i][l0:l1]))
        return rows

    def update_metrics(self, preds, batch):
        """val.py:72-116 for the whole batch in one launch.  preds: postprocess' (rows [B, max_det, >= 6], counts [B]) pair, or a list of
        per-image [n, >= 6] tensors (non_max_suppression)."""
        dev = self.device
        if isinstance(preds, tuple) and len(preds) == 2 and torch.is_tensor(preds[0]) and preds[0].dim() == 3:
            det, cnt, lens = preds[0].float().contiguous(), preds[1], None
        else:
            lens = [int(p.shape[0]) for p in preds]
            det = torch.zeros((len(preds), max(lens + [1]), preds[0].shape[1] if len(preds) else 6), dtype=torch.float32, device=dev)
            for i, p in enumerate(preds):
                if lens[i]:
                    det[i, :lens[i]] = p
            cnt = torch.tensor(lens, dtype=torch.int32).to(dev)
        B = det.shape[0]
        height, width = batch["img"].shape[2:]
        single = self._flag("single_cls")
        # the labels sorted by image (stable: the order inside an image stays), on whichever device they live
        bi = batch["batch_idx"].reshape(-1).float()
        order = torch.argsort(bi, stable=True)
        loff = torch.searchsorted(bi[order].contiguous(), torch.arange(B + 1, dtype=torch.float32, device=bi.device)).to(torch.int32)
        tcls = batch["cls"].reshape(-1).float()[order.to(batch["cls"].device)]
        lxywh = batch["bboxes"].reshape(-1, 4).float()[order.to(batch["bboxes"].device)]
        rec = torch.tensor([scale_record((height, width), batch["ori_shape"][si] if "ori_shape" in batch else (height, width),
                                         batch["ratio_pad"][si] if "ratio_pad" in batch else None) for si in range(B)],
                           dtype=torch.float32).view(B, 5).to(dev)
        lcls, loff_d = tcls.to(dev), loff.to(dev)
        cm = self.confusion_matrix
        correct, predn, tboxn = kops.val_box_match(det, cnt, lcls, lxywh.to(dev), loff_d, (height, width), rec, self._iouv_dev, single,
                                                   self._confusion, cm.conf, cm.iou_thres)
        ctx = SimpleNamespace(det=det, cnt=cnt, lens=lens, lcls=lcls, loff=loff_d, order=order, height=height, width=width,
                              loff_h=None if loff.is_cuda else loff.tolist())
        task = self._task_correct(batch, ctx) if self.n_task else ()
        cc = det[:, :, 4:6].contiguous()
        if single:
            cc[:, :, 1] = 0
        self._pending.append(dict(correct=(correct, *task), cc=cc, cnt=cnt, lens=lens, tcls=tcls, loff=loff, loff_h=ctx.loff_h))
        self.seen += B
        save_json = self._flag("save_json") and self.n_task == 0
        if self._flag("save_txt") or save_json:
            self._save_predictions(batch, torch.cat((predn, cc), 2), cnt if lens is None else lens, save_json)

    def _task_correct(self, batch, ctx):
        """The task's own `correct` matrices of the batch: uint8 [B, max_det, niou] device tensors, `n_task` of them."""
        return ()

    def _match_iou(self, mats, ctx):
        """One dy_val_iou_match for the batch: mats[b] = the device IoU matrix [labels of image b, its detections], or None for an image
        without labels or without detections."""
        dev = self.device
        sizes = [0 if m is None else m.numel() for m in mats]
        moff = torch.tensor([sum(sizes[:b]) for b in range(len(mats))], dtype=torch.int64).to(dev)
        live = [m.reshape(-1) for m in mats if m is not None and m.numel()]
        flat = torch.cat(live) if live else torch.zeros(1, dtype=torch.float32, device=dev)
        return kops.val_iou_match(flat.float().contiguous(), moff, ctx.det, ctx.cnt, ctx.lcls, ctx.loff, self._iouv_dev,
                                  self._flag("single_cls"))

    def _save_predictions(self, batch, predn, counts, save_json):
        """save_txt -> save_dir/labels/<stem>.txt, save_json -> records for save_dir/predictions.json (val.py:111-116).  This is the one
        place where a batch's predictions are read back inside the loop."""
        if "im_file" not in batch or self.save_dir is None:
            raise ValueError("save_txt / save_json need the batch's 'im_file' names and a save_dir (save_dir=, or project= / name=)")
        predn = predn.cpu()
        counts = counts.tolist() if torch.is_tensor(counts) else counts
        height, width = batch["img"].shape[2:]
        if self._flag("save_txt"):
            (self.save_dir / "labels").mkdir(parents=True, exist_ok=True)
        for si, n in enumerate(counts):
            if n == 0:
                continue
            if save_json:
                self.jdict.extend(pred_to_json(predn[si, :n], batch["im_file"][si]))
            if self._flag("save_txt"):
                shape = batch["ori_shape"][si] if "ori_shape" in batch else (height, width)
                save_one_txt(predn[si, :n], self._flag("save_conf"), shape, self.save_dir / "labels" / f"{Path(batch['im_file'][si]).stem}.txt")

    def get_stats(self):
        """val.py:118-129: the one read-back of the run (the queued `correct` / confidence / class tensors and the confusion matrix)."""
        rows = self.stats
        self.confusion_matrix.matrix = self._confusion.cpu().numpy().astype(np.float64)
        self.metrics.confusion_matrix = self.confusion_matrix
        if self._flag("save_json") and self.n_task == 0 and self.jdict:
            self.save_dir.mkdir(parents=True, exist_ok=True)
            with open(self.save_dir / "predictions.json", "w") as f:
                json.dump(self.jdict, f)
        if not rows:
            self.nt_per_class = np.zeros(self.nc, dtype=int)
            return self.metrics.results_dict
        stats = [torch.cat(x, 0).numpy() for x in zip(*rows)]
        if len(stats) and stats[0].any():
            self.metrics.process(*stats)
        self.nt_per_class = np.bincount(stats[-1].astype(int), minlength=self.nc)
        return self.metrics.results_dict

    def print_results(self):
        """val.py:131-142: the `all` row, then with `verbose`, outside training and nc > 1 one row per class that has labels."""
        pf = "%22s" + "%11i" * 2 + "%11.3g" * len(self.metrics.keys)
        LOGGER.info(pf % ("all", self.seen, self.nt_per_class.sum(), *self.metrics.mean_results()))
        if self.nt_per_class.sum() == 0:
            LOGGER.warning(f"WARNING no labels found in {getattr(self.args, 'task', 'detect')} set, can not compute metrics without labels")
        if self._flag("verbose", True) and not self.training and self.nc > 1 and len(self.stats):
            for i, c in enumerate(self.metrics.ap_class_index):
                LOGGER.info(pf % (self.names[c], self.seen, self.nt_per_class[c], *self.metrics.class_result(i)))

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
        self.print_results()
        model.train(was_training)
        return {k: float(v) for k, v in stats.items()}


class SegmentationValidator(DetectionValidator):
    """Segment validator (reference models/yolo/segment/val.py): NMS with the mask-coefficient columns, predicted masks of the whole
    batch in one launch, mask IoU against the gt masks with integer counts (dy_seg_mask_iou), the box `correct` matrices and the
    confusion matrix from dy_val_box_match, the mask ones from one dy_val_iou_match on the batch's mask-IoU matrices, SegmentMetrics.
    `process` as in init_metrics (val.py:31-39): save_json False -> process_mask at the
    proto resolution (dy_seg_mask_decode), save_json True -> process_mask_upsample at the input resolution
    (dy_seg_mask_upsample).  gt masks (index maps or planes) at another resolution than the predicted masks are resized
    bilinearly and thresholded at 0.5 (val.py:146-148; dy_mask_resize).  Writing predictions.json itself (RLE through pycocotools,
    scale_image through cv2) is out of scope: save_json only selects the masks that are evaluated."""

    n_task = 1

    def __init__(self, args=None, dataloader=None, save_dir=None):
        super().__init__(args, dataloader, save_dir)
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

    def _task_correct(self, batch, ctx):
        masks = batch["masks"]
        loff = ctx.loff_h if ctx.loff_h is not None else ctx.loff.tolist()
        mats = []
        for si, n in enumerate(ctx.lens):
            m = loff[si + 1] - loff[si]
            if n == 0 or m == 0:
                mats.append(None)
                continue
            overlap = bool(getattr(self.args, "overlap_mask", True))
            gt = masks[si] if overlap else masks[ctx.order[loff[si]:loff[si + 1]].to(masks.device)]
            pred = batch["pmasks"][si]
            if tuple(gt.shape[-2:]) != tuple(pred.shape[-2:]):
                gt = ops.resize_masks(gt, pred.shape[-2:], m=m if overlap else None)       # -> uint8 planes [m, h, w]
                overlap = False
            mats.append(ops.mask_iou_binary(gt, pred, overlap, m))
        return (self._match_iou(mats, ctx),)


class PoseValidator(DetectionValidator):
    """Pose validator (reference models/yolo/pose/val.py): NMS with multi_label and the K * ndim keypoint columns appended,
    boxes (scale_boxes) and keypoints (scale_coords) to ori_shape / ratio_pad, OKS against the gt keypoints in native space with
    area = gt box w * h * 0.53 (kpt_iou on dy_kpt_oks), the box `correct` matrices and the confusion matrix from dy_val_box_match, the
    pose ones from one dy_val_iou_match on the batch's OKS matrices, PoseMetrics.  sigma = metrics.oks_sigmas(kpt_shape)."""

    n_task = 1

    def __init__(self, args=None, dataloader=None, save_dir=None):
        super().__init__(args, dataloader, save_dir)
        self.args.task = "pose"
        self.metrics = PoseMetrics()

    def init_metrics(self, model):
        super().init_metrics(model)
        self.kpt_shape = list(model.model[-1].kpt_shape)
        self.sigma = oks_sigmas(self.kpt_shape)

    def postprocess(self, preds):
        return super().postprocess(preds, nc=self.nc)

    def update_metrics(self, preds, batch):
        """val.py:62-109: the keypoints are scaled on host copies (one per batch), the OKS matrices stay on the device."""
        if "keypoints" not in batch:
            raise ValueError("pose validation: the batch has no 'keypoints'")
        super().update_metrics(preds, dict(batch, keypoints=batch["keypoints"].cpu().float()))

    def _task_correct(self, batch, ctx):
        height, width = ctx.height, ctx.width
        loff = ctx.loff_h if ctx.loff_h is not None else ctx.loff.tolist()
        order, pred_h = ctx.order.cpu(), ctx.det.cpu()
        box_all = batch["bboxes"].cpu().float()
        mats = []
        for si, n in enumerate(ctx.lens):
            m = loff[si + 1] - loff[si]
            if n == 0 or m == 0:
                mats.append(None)
                continue
            idx = order[loff[si]:loff[si + 1]]
            shape = batch["ori_shape"][si] if "ori_shape" in batch else (height, width)
            ratio_pad = batch["ratio_pad"][si] if "ratio_pad" in batch else None
            kpts = batch["keypoints"][idx]
            nk = kpts.shape[1] if kpts.dim() == 3 else int(self.kpt_shape[0])
            pred_kpts = pred_h[si, :n, 6:].clone().view(n, nk, -1)
            ops.scale_coords((height, width), pred_kpts, shape, ratio_pad=ratio_pad)
            tkpts = kpts.clone()
            tkpts[..., 0] *= width
            tkpts[..., 1] *= height
            tkpts = ops.scale_coords((height, width), tkpts, shape, ratio_pad=ratio_pad)
            tbox = ops.xywh2xyxy(box_all[idx]) * torch.tensor((width, height, width, height), dtype=torch.float32)
            ops.scale_boxes((height, width), tbox, shape, ratio_pad=ratio_pad)
            area = ops.xyxy2xywh(tbox)[:, 2:].prod(1) * 0.53
            mats.append(kpt_iou(tkpts.to(self.device), pred_kpts.to(self.device), area, self.sigma))
        return (self._match_iou(mats, ctx),)


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

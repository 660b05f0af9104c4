"""`YOLO` facade with the reference call surface (ultralytics/engine/model.py:29-416): YOLO(model), .train(**kw), .val(**kw),
.load(), .fuse(); the detect, segment, pose and classify tasks."""
from pathlib import Path

import torch

from ..nn.tasks import all_tasks
from .trainer import DetectionTrainer, get_cfg


def _model_class(task):
    return all_tasks()[task][0]


def _resolve_task(task, d):
    """The yaml's own task unless one is given; 'pose' and a Pose head go together only, and so do 'classify' and a Classify
    head (an explicit task that contradicts them raises, as one outside the hot path does)."""
    from ..nn.tasks import guess_model_task
    head = guess_model_task(d)
    if task is not None and any((task == t) != (head == t) for t in ("pose", "classify")):
        raise NotImplementedError(f"task '{task}' does not match the model's {head} head")
    return task or head


def segment_postprocess(dets, proto, input_shape, orig_shapes=None, retina_masks=False, names=None):
    """SegmentationPredictor.postprocess after its NMS (reference models/yolo/segment/predict.py:25-44): dets = one [n_i, 6 + nm]
    tensor per image (non_max_suppression), proto [B, nm, mh, mw], input_shape = the network input (h, w) -> one `Results` per image.
    retina_masks=False: masks at the input resolution (process_mask, upsample=True), then the boxes scaled to orig_shapes[i];
    retina_masks=True: the boxes scaled first, then masks at orig_shapes[i] (process_mask_native).  The masks of the whole batch come
    from one process_masks_batched call (one launch per distinct output shape); an image without detections has masks None.
    `Masks.data` is f32 0 / 1 like the reference's; the uint8 planes the kernel writes are converted last."""
    from ..utils import ops as uops
    from .results import Results
    H, W = int(input_shape[0]), int(input_shape[1])
    shapes = [tuple(int(v) for v in s[:2]) for s in orig_shapes] if orig_shapes is not None else [(H, W)] * len(dets)
    dets = [d.clone() for d in dets]
    if retina_masks:
        for d, shape in zip(dets, shapes):
            uops.scale_boxes((H, W), d[:, :4], shape)
        masks = uops.process_masks_batched(proto, dets, (H, W), mode="native", out_shapes=shapes)
    else:
        masks = uops.process_masks_batched(proto, dets, (H, W), mode="input")
        for d, shape in zip(dets, shapes):
            uops.scale_boxes((H, W), d[:, :4], shape)
    return [Results(shape, d[:, :6], names=names, masks=m.float() if len(d) else None) for d, m, shape in zip(dets, masks, shapes)]


class YOLO:
    def __init__(self, model="yolov8l.yaml", task=None):
        if task not in (None, "detect", "segment", "pose", "classify"):
            raise NotImplementedError("only the detect, segment, pose and classify tasks are on the Dedark-YOLO hot path")
        self.task = task
        self.trainer = None
        self.validator = None
        self.overrides = {}
        suffix = Path(str(model)).suffix
        if suffix == ".yaml":
            self._new(model)
        elif suffix in (".pt", ".pth"):
            self._load(model)
        else:
            raise FileNotFoundError(f"'{model}': expected a model .yaml or a state_dict checkpoint .pt")

    def _new(self, cfg):
        from ..nn.tasks import yaml_model_load
        self.cfg = cfg
        d = yaml_model_load(cfg)
        self.task = _resolve_task(self.task, d)
        self.model = _model_class(self.task)(d)
        self.overrides["model"] = cfg
        self.overrides["task"] = self.task

    def _load(self, weights):
        """reference nn/tasks.py:592-630,674-707 (attempt_load_one_weight): `ckpt.get('ema') or ckpt['model']`, cast to fp32.  Reads
        both this package's state_dict checkpoints and the reference's pickled-module last.pt / best.pt (utils/checkpoint.py)."""
        from ..utils.checkpoint import load_checkpoint
        ck = load_checkpoint(weights)
        cfg = ck.yaml
        if cfg is None:
            raise RuntimeError(f"{weights}: the checkpoint carries no model yaml")
        from ..nn.tasks import yaml_model_load
        d = cfg if isinstance(cfg, dict) else yaml_model_load(cfg)
        self.task = _resolve_task(self.task, d)
        self.model = _model_class(self.task)(d, nc=ck.nc)
        self.overrides["task"] = self.task
        n = self.model.load(ck.state_dict)
        if n == 0:
            raise RuntimeError(f"{weights}: no tensor of the checkpoint matches the graph of its yaml")
        if isinstance(ck.names, dict) and len(ck.names) == len(self.model.names):
            self.model.names = {int(k): str(v) for k, v in ck.names.items()}
        self.ckpt = ck
        self.cfg = cfg
        self.overrides["model"] = cfg

    def __call__(self, source, **kw):
        return self.predict(source, **kw)

    def load(self, weights):
        self.model.load(weights)
        return self

    def fuse(self):
        self.model.fuse()
        return self

    def _attach_data(self, data):
        """What the reference trainer's get_model / set_model_attributes do with the data dict (models/yolo/detect/train.py:104-121,
        pose/train.py:33-46): a model whose class count (pose: kpt_shape) differs from the dataset's is rebuilt from its yaml with the
        dataset's -- tensors that keep their shape are carried over, as a pretrained load does -- then `names` (pose: `kpt_shape`)
        are attached."""
        nc, kpt = int(data["nc"]), data.get("kpt_shape")
        rebuild = nc != int(self.model.yaml["nc"])
        kw = {}
        if self.task == "pose" and kpt is not None:
            kw["data_kpt_shape"] = list(kpt)
            rebuild = rebuild or list(kpt) != list(self.model.yaml["kpt_shape"])
        if rebuild:
            from copy import deepcopy
            dev = next(self.model.parameters()).device
            old = self.model
            self.model = _model_class(self.task)(deepcopy(old.yaml), nc=nc, **kw).to(dev)
            if getattr(self, "ckpt", None) is not None:
                self.model.load(old.state_dict())
        self.model.names = dict(data["names"])
        if self.task == "pose" and kpt is not None:
            self.model.kpt_shape = list(kpt)

    def _data_args(self, kwargs):
        ov = dict(self.overrides)
        ov.update(kwargs)
        return get_cfg(ov)

    def _cls_imgsz(self, kwargs):
        """the classify task's image size for the paths that read images from disk: 224 unless the call or the overrides give one
        (reference models/yolo/classify/train.py:22-23)"""
        if kwargs.get("imgsz") is None and self.overrides.get("imgsz") is None:
            return dict(kwargs, imgsz=224)
        return kwargs

    def train(self, loader=None, save_dir=None, **kwargs):
        """A classify model takes `data=<dataset directory>` (train/<class>/..., val/ or test/ likewise: data.check_cls_dataset,
        ClassifyTrainLoader, ClassifyValLoader; imgsz 224 unless given; the head is rebuilt for the dataset's class count).
        model.train(data='dataset/data.yaml', epochs=..., imgsz=..., batch=..., ...): the training set of the data yaml through
        data.build_train_loader (labels read and verified, images decoded once, augmentation on the device) and, with `val: True`, its
        val split through data.build_val_loader at twice the batch (the reference's trainer does the same) for the per-epoch
        validation.  Checkpoints are written to `save_dir`, or to project/name when either is given; otherwise nothing is written.
        `loader=<iterable of reference-schema batch dicts>` instead of `data=` is the path for batches that are already in memory."""
        cls_data = self.task == "classify" and loader is None
        args = self._data_args(self._cls_imgsz(kwargs) if cls_data else kwargs)
        self.trainer = DetectionTrainer(args)
        if loader is not None:
            self.trainer.setup(self.model, total_iterations=len(loader) * self.trainer.args.epochs)
            return self.trainer.train(loader)
        if not getattr(args, "data", None):
            raise ValueError("pass data=<path to a data yaml> (the dataset is read from disk) or loader=<iterable of batch dicts>")
        from ..data import (build_cls_train_loader, build_cls_val_loader, build_train_loader, build_val_loader, check_cls_dataset,
                            check_det_dataset)
        # classify: `data` is a directory with one folder per class under train/ and val/ or test/ (check_cls_dataset)
        data = check_cls_dataset(args.data) if cls_data else check_det_dataset(args.data)
        self._attach_data(data)
        tr = self.trainer
        torch.cuda.set_device(tr.device)                      # the loaders launch their resize kernels on the current device's stream
        if cls_data:
            loader = build_cls_train_loader(args, data, tr.device, tr.rank, tr.world_size)
        else:
            loader = build_train_loader(args, data, self.task, tr.device, tr.rank, tr.world_size)
        if len(loader) == 0:
            raise ValueError(f"the training set holds {len(loader.shapes)} images, fewer than one batch of {args.batch}")
        tr.setup(self.model, total_iterations=len(loader) * args.epochs)
        val_loader = None
        if getattr(args, "val", True) and tr.rank in (-1, 0) and cls_data:
            val_loader = build_cls_val_loader(args, data, tr.device, "val", batch=2 * int(args.batch))
        elif getattr(args, "val", True) and tr.rank in (-1, 0):
            stride = max(int(self.model.stride.max()), 32)
            val_loader = build_val_loader(args, data, self.task, tr.device, "val", batch=2 * int(args.batch), stride=stride)
        if save_dir is None and (getattr(args, "project", None) or getattr(args, "name", None)):
            save_dir = Path(args.project or "runs") / (args.name or "train")
        return tr.train(loader, val_loader=val_loader, save_dir=save_dir)

    def val(self, loader=None, **kwargs):
        """model.val(data='dataset/data.yaml', split='val', ...): the split as rect batches of the cfg's `batch` (data.DeviceValLoader);
        `loader=` as before.  The model must be on the GPU."""
        cls_data = self.task == "classify" and loader is None
        args = self._data_args(self._cls_imgsz(kwargs) if cls_data else kwargs)
        if loader is None and getattr(args, "data", None):
            from ..data import build_cls_val_loader, build_val_loader, check_cls_dataset, check_det_dataset
            split = getattr(args, "split", None) or "val"
            # classify: a dataset directory; 'val' falls back to test/ and 'test' to val/ (check_cls_dataset)
            data = check_cls_dataset(args.data, split) if cls_data else check_det_dataset(args.data)
            dev = next(self.model.parameters()).device
            if len(data["names"]) != len(self.model.names):
                raise ValueError(f"val(data=): the dataset has {len(data['names'])} classes, the model {len(self.model.names)}: "
                                 "their class ids do not mean the same")
            self.model.names = dict(data["names"])
            torch.cuda.set_device(dev)
            if cls_data:
                loader = build_cls_val_loader(args, data, dev, split)
            else:
                loader = build_val_loader(args, data, self.task, dev, split, stride=max(int(self.model.stride.max()), 32))
        self.validator = all_tasks()[self.task][2](args)        # kept: confusion_matrix, nt_per_class, stats, print_results()
        return self.validator(self.model, loader)

    @torch.no_grad()
    def predict(self, source, conf=0.25, iou=0.7, max_det=300, agnostic_nms=False, orig_shapes=None, retina_masks=None, augment=False,
                **kw):
        """reference engine/predictor.py stream_inference + DetectionPredictor.postprocess (models/yolo/detect/predict.py:12-38).
        `source` is either
          * an already letter-boxed batch: a uint8 [B,3,H,W] RGB tensor (or float in [0,1]); boxes are scaled back to `orig_shapes[i]`
            (default: the network input shape); or
          * an image file, a directory of images, or a list of files / decoded uint8 HWC BGR arrays: every image is letter-boxed on the
            device to the stride-multiple shape of its own aspect ratio (data.augment.letterbox_auto: the predictor's
            LetterBox(imgsz, auto=True), scaleup, linear resize; `imgsz=` in the call or the cfg's), one image per forward (files are
            decoded one at a time); `orig_shapes` is filled from the images and `Results.path` from the files.  A classify model
            centre-crops and resizes instead (_predict_classify) and forwards chunks of the cfg's `batch`.
        Returns one `Results` per image.  A segment model also fills
        `Results.masks` (segment_postprocess; `retina_masks` defaults to the cfg's).  Plotting
        and the mask contours (`Masks.xy`) are outside the hot path.  A classify model returns `Results.probs` (the eval soft-max row
        of each image; classify/predict.py:23-31) and no boxes.  `augment=True`: multi-scale, flipped inference (DetectionModel._predict_augment) before the NMS."""
        if torch.is_tensor(source):
            return self._predict_batch(source, conf, iou, max_det, agnostic_nms, orig_shapes, retina_masks, augment)
        import numpy as np
        from ..data.augment import letterbox_auto
        from ..data.dataset import decode, get_img_files
        dev = next(self.model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("predict() needs the model on a GPU (there is no CPU path)")
        items = source if isinstance(source, (list, tuple)) else [source]
        images, paths = [], []
        for it in items:
            if isinstance(it, np.ndarray):
                if it.dtype != np.uint8 or it.ndim != 3 or it.shape[2] != 3:
                    raise ValueError("predict(): an image array must be uint8 HWC with 3 channels (BGR, as cv2.imread gives it)")
                images.append(np.ascontiguousarray(it))
                paths.append(None)
            else:
                files = get_img_files(str(it)) if Path(str(it)).is_dir() else [str(it)]
                images += files                                # decoded one at a time, below
                paths += files
        if self.task == "classify":
            return self._predict_classify(images, paths, kw, dev, decode)
        imgsz = int(kw.get("imgsz") or getattr(get_cfg(dict(self.overrides)), "imgsz", 640))
        stride = max(int(self.model.stride.max()), 32)
        out = []
        for im in images:                                     # one image per forward, as the reference's file stream (batch 1) runs
            im = decode(im) if isinstance(im, str) else im
            boxed = letterbox_auto(torch.from_numpy(im).to(dev), imgsz, stride)[0]
            out += self._predict_batch(boxed[None], conf, iou, max_det, agnostic_nms, [tuple(im.shape[:2])], retina_masks, augment)
        for r, p in zip(out, paths):
            r.path = p
        return out

    def _predict_classify(self, images, paths, kw, dev, decode):
        """predict() of a classify model for files / arrays: the predictor's transform (classify/predict.py:18-21 = classify_transforms:
        CenterCrop(imgsz) + ToTensor) -- data.augment.center_crop_batch, one dy_cls_render launch per chunk -- and one forward per
        chunk of the cfg's `batch` images; imgsz 224 unless the call or the overrides give one."""
        from ..data.augment import center_crop_batch
        args = get_cfg(dict(self.overrides))
        imgsz = int(self._cls_imgsz(kw).get("imgsz") or args.imgsz)
        step, out = max(int(getattr(args, "batch", 1) or 1), 1), []
        torch.cuda.set_device(dev)
        for o in range(0, len(images), step):
            chunk = [decode(im) if isinstance(im, str) else im for im in images[o:o + step]]
            batch = center_crop_batch([torch.from_numpy(im).to(dev) for im in chunk], imgsz)
            out += self._predict_batch(batch, None, None, None, None, [tuple(im.shape[:2]) for im in chunk], None, False)
        for r, p in zip(out, paths):
            r.path = p
        return out

    def _predict_batch(self, source, conf, iou, max_det, agnostic_nms, orig_shapes, retina_masks, augment):
        """predict() for a letter-boxed tensor batch"""
        from ..utils import ops as uops
        from .results import Results
        from .validator import DetectionValidator
        dev = next(self.model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("predict() needs the model on a GPU (there is no CPU path)")
        was_training = self.model.training
        self.model.eval()
        if source.dtype == torch.uint8:
            v = DetectionValidator(get_cfg(dict(self.overrides)))
            v.device = dev
            img = v.preprocess(dict(img=source))["img"]
        else:
            img = source.to(dev).float()
        preds = self.model(img, augment=bool(augment))        # engine/predictor.py:167 (detect models only; the others warn)
        if self.task == "classify":
            H, W = img.shape[2:]
            out = [Results(tuple(orig_shapes[i]) if orig_shapes is not None else (H, W), names=self.model.names, probs=p)
                   for i, p in enumerate(preds)]
            self.model.train(was_training)
            return out
        if self.task == "segment":                            # models/yolo/segment/predict.py:16-26
            dets = uops.non_max_suppression(preds[0], conf, iou, agnostic=agnostic_nms, max_det=max_det, nc=len(self.model.names))
            proto = preds[1][-1] if len(preds[1]) == 3 else preds[1]
            if retina_masks is None:
                retina_masks = bool(getattr(get_cfg(dict(self.overrides)), "retina_masks", False))
            out = segment_postprocess([d[:, :6 + proto.shape[1]] for d in dets], proto, img.shape[2:], orig_shapes, retina_masks,
                                      self.model.names)
            self.model.train(was_training)
            return out
        pose = self.task == "pose"
        nc = self.model.model[-1].nc if pose else 0
        dets = uops.non_max_suppression(preds, conf, iou, agnostic=agnostic_nms, max_det=max_det, nc=nc)
        H, W = img.shape[2:]
        out = []
        for i, d in enumerate(dets):
            shape = tuple(orig_shapes[i]) if orig_shapes is not None else (H, W)
            d = d.clone()
            uops.scale_boxes((H, W), d[:, :4], shape)          # also clips to the image, like predict.py:27
            kpts = None
            if pose:                                          # models/yolo/pose/predict.py:29-30
                kpts = uops.scale_coords((H, W), d[:, 6:].reshape(len(d), *self.model.model[-1].kpt_shape), shape)
            out.append(Results(shape, d[:, :6], names=self.model.names, keypoints=kpts))
        self.model.train(was_training)
        return out

    def save(self, path):
        torch.save(dict(state_dict=self.model.state_dict(), yaml=self.model.yaml, nc=self.model.yaml["nc"]), path)

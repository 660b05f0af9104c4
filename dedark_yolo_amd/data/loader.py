"""Batches of the device input pipeline for the training loop: what `build_dataloader` + the dataloader workers are in the
reference (ultralytics/data/build.py:72-109, dataset.py:171-188), with the decoded images kept in device memory.

`DeviceAugmentLoader` owns the decoded uint8 images.  `resident=True` (the MI355X-sized default: 288 GB of HBM holds a VOC-scale dataset
several times over -- 16.5 k images x ~0.9 MB) keeps them in HBM, so a step reads nothing over PCIe; `resident=False` keeps them in pinned
host memory and uploads the source images of batch i+1 on a copy stream while step i runs (the PCIe-inclusive mode bench.py reports).
Either way the augmented pixels are produced on the device by ONE launch per batch (DeviceAugmenter.render)."""
import math
import random as _random

import numpy as np
import torch

from .augment import (N_RESAMPLE, AugmentHyp, DeviceAugmenter, TaskLabels, instance_offsets, pack_polygons, pack_rows, plan_train_sample,
                      polygon_masks)


class DeviceAugmentLoader:
    """task="detect": batches of {img, batch_idx, cls, bboxes, n_max}.  task="segment" (labels carry `segments`): `masks` is added --
    rasterised on the device from the augmented polygons (csrc/polymask.hip) -- and batch_idx / cls / bboxes are the device rows in the
    area order the overlap masks index (`sorted_idx`: the permutation).  task="pose" (labels carry `keypoints`): `keypoints` [N, K, 3]
    f32 is added.  Everything is uploaded from the pinned ring and issued on the loader's stream.

    hyp.mixup > 0: MixUp (ultralytics/data/augment.py:272-288) -- a second planned image per mixed sample is warped and blended in by the
    same launch (dy_aug_mosaic_warp_mix) and its labels are appended to the primary's.  `close_mosaic()` switches mosaic / mixup /
    copy_paste off from the next epoch on (the reference's trainer does that for the last `close_mosaic` epochs).  The non-mosaic path
    (hyp.mosaic < 1, and every sample after close_mosaic) pads an image as it is: it needs every image at its load_image size (long
    side == imgsz) and raises NotImplementedError otherwise."""

    def __init__(self, images, labels, imgsz, batch_size, hyp=None, device="cuda", resident=True, seed=0, shuffle=True, drop_last=True,
                 task="detect", flip_idx=None, mask_ratio=4, overlap_mask=True):
        self.device = torch.device(device)
        self.imgsz, self.bs, self.hyp = int(imgsz), int(batch_size), hyp or AugmentHyp()
        self.labels = labels
        self.extras = TaskLabels(labels, task, self.hyp, flip_idx, mask_ratio, overlap_mask, self.imgsz)
        self.hyp, self.task = self.extras.hyp, task           # a pose set without flip_idx: fliplr = 0 (v8_transforms)
        self.resident = bool(resident)
        self.shapes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
        self.shuffle, self.drop_last = shuffle, drop_last
        self.rnd = _random.Random(seed)                      # own generators: the loader must not disturb the caller's global RNG state
        self.nprnd = np.random.RandomState(seed + 1)
        if self.resident:
            self.aug = DeviceAugmenter(images, [dict(cls=l["cls"], bboxes=l["bboxes"]) for l in labels], imgsz, self.hyp, device)
            self.host = None
        else:
            self.host = [(im if torch.is_tensor(im) else torch.from_numpy(np.ascontiguousarray(im))).pin_memory() for im in images]
            self.aug = None
        self.uploaded_bytes = 0
        self._close = False

    def close_mosaic(self):
        """BaseTrainer's `close_mosaic` switch (engine/trainer.py:302-308 -> YOLODataset.close_mosaic, data/dataset.py:152-157): from the
        next __iter__ on, mosaic = mixup = copy_paste = 0 on the loader's OWN copy of the hyper-parameters (the caller's object is left
        alone).  A batch already prepared keeps its plans."""
        self._close = True

    def _apply_close(self):
        import copy
        hyp = copy.copy(self.hyp)
        hyp.mosaic = hyp.mixup = hyp.copy_paste = 0.0
        self.hyp = self.extras.hyp = hyp
        if self.aug is not None:
            self.aug.hyp = hyp
        self._close = False

    def __len__(self):
        n = len(self.shapes)
        return n // self.bs if self.drop_last else -(-n // self.bs)

    def _plans(self, indices):
        buf = list(range(len(self.shapes)))
        return [plan_train_sample(i, self.shapes, buf, self.imgsz, self.hyp, self.rnd, self.nprnd) for i in indices]

    RING = 3                                                  # staging buffers in flight (pinned host memory is expensive to allocate)

    def _slots(self):
        from .augment import descriptor_bytes
        if getattr(self, "_ring", None) is None:
            cap = 64 * self.bs                                   # label rows per batch the pinned buffer holds (grown on demand)
            self._ring = [dict(desc=torch.empty(self.bs * descriptor_bytes(self.hyp.mixup > 0), dtype=torch.uint8).pin_memory(),
                               lab=torch.empty((cap, 6), dtype=torch.float32).pin_memory(), ev=torch.cuda.Event()) for _ in range(self.RING)]
            self._turn = 0
            self.stream = torch.cuda.Stream(device=self.device)
        slot = self._ring[self._turn % self.RING]
        self._turn += 1
        slot["ev"].synchronize()                                 # its last copies (three batches ago) have long finished
        return slot

    def _prepare(self, indices):
        """One whole batch -- plans, label bookkeeping, descriptor / label / (host mode) image uploads from pinned memory, the render
        launch -- on the loader's own stream, without a host synchronisation: it is issued while the previous training step is still
        running on the compute stream and shares the GPU with it.  Returns (batch dict of device tensors, event)."""
        plans = self._plans(indices)
        lab = [self.extras.train_labels(p, self.shapes) for p in plans]
        n = sum(len(l[0]) for l in lab)
        slot = self._slots()
        if n > slot["lab"].shape[0]:
            slot["lab"] = torch.empty((2 * n, 6), dtype=torch.float32).pin_memory()
        pack_rows(lab, slot["lab"].numpy())
        extra = None
        if self.task == "segment":                               # polygons + per-image offsets ride in the same pinned slot
            if "off" not in slot:
                slot["off"] = torch.empty(self.bs + 1, dtype=torch.int32).pin_memory()
            if slot.get("poly") is None or n > slot["poly"].shape[0]:
                slot["poly"] = torch.empty((max(2 * n, 16 * self.bs), N_RESAMPLE, 2), dtype=torch.int16).pin_memory()
            pack_polygons(lab, slot["poly"].numpy())
            slot["off"].numpy()[:len(lab) + 1] = instance_offsets(lab)
        elif self.task == "pose":
            K = lab[0][2].shape[1]
            if slot.get("kp") is None or n > slot["kp"].shape[0] or slot["kp"].shape[1] != K:
                slot["kp"] = torch.empty((max(2 * n, 16 * self.bs), K, 3), dtype=torch.float32).pin_memory()
            kph, o = slot["kp"].numpy(), 0
            for l in lab:
                kph[o:o + len(l[0])] = l[2]
                o += len(l[0])
        with torch.cuda.stream(self.stream):
            if self.resident:
                aug = self.aug
            else:
                need = sorted({s for p in plans for q in (p, p.mix) if q is not None for s in q.sources})
                dev = {s: self.host[s].to(self.device, non_blocking=True) for s in need}
                self.uploaded_bytes += sum(self.host[s].numel() for s in need)
                aug = DeviceAugmenter.__new__(DeviceAugmenter)           # a view of the uploaded subset with the full index space
                aug.device, aug.imgsz, aug.hyp, aug.images = self.device, self.imgsz, self.hyp, _Sparse(dev)
            img = aug.render(plans, staging=slot["desc"])
            labd = slot["lab"][:n].to(self.device, non_blocking=True)
            if self.task == "segment":
                polyd = slot["poly"][:n].to(self.device, non_blocking=True)
                offd = slot["off"][:len(lab) + 1].to(self.device, non_blocking=True)
                masks, rows, perm = polygon_masks(polyd, offd, labd, len(lab), self.imgsz, self.imgsz, self.extras.mask_ratio,
                                                  self.extras.overlap_mask)
                extra = dict(masks=masks)
                tensors = (img, labd, polyd, offd, masks)
                if self.extras.overlap_mask:
                    labd, extra["sorted_idx"] = rows, perm
                    tensors += (rows, perm)
            elif self.task == "pose":
                kpd = slot["kp"][:n].to(self.device, non_blocking=True)
                extra, tensors = dict(keypoints=kpd), (img, labd, kpd)
            else:
                tensors = (img, labd)
            slot["ev"].record(self.stream)
        batch = dict(img=img, batch_idx=labd[:, 0], cls=labd[:, 1:2], bboxes=labd[:, 2:6], n_max=max([len(l[0]) for l in lab] + [0]))
        if extra:
            batch.update(extra)
        return batch, slot["ev"], tensors

    def __iter__(self):
        if self._close:
            self._apply_close()
        order = list(range(len(self.shapes)))
        if self.shuffle:
            self.rnd.shuffle(order)
        chunks = [order[i:i + self.bs] for i in range(0, len(order), self.bs)]
        if self.drop_last:
            chunks = [c for c in chunks if len(c) == self.bs]
        nxt = self._prepare(chunks[0]) if chunks else None
        for k in range(len(chunks)):
            batch, ev, tensors = nxt
            cur = torch.cuda.current_stream()
            cur.wait_event(ev)
            for t in tensors:
                t.record_stream(cur)                             # allocated on the loader stream, consumed (and freed) on the compute stream
            # batch k+1 is prepared when the consumer comes back for it, i.e. right after step k has been ISSUED: the host work and the
            # uploads / render on the loader stream overlap step k on the GPU
            yield batch
            nxt = self._prepare(chunks[k + 1]) if k + 1 < len(chunks) else None


class _Sparse:
    """list-like over the uploaded subset of the dataset"""

    def __init__(self, d):
        self.d = d

    def __getitem__(self, i):
        return self.d[i]


# ---------------------------------------------------------------------------------------------------------------- datasets from disk
def _device_images(decoded, imgsz, device, augment, keep_on_device=True):
    """decoded uint8 HWC BGR arrays brought to their load_image size on the device (base.py:142-157: linear for training, area for a
    validation image that shrinks): list of uint8 HWC tensors, on the device or (keep_on_device=False) copied back to the host"""
    from .augment import load_resize
    out = []
    for im in decoded:
        t = load_resize(torch.from_numpy(im).to(device), imgsz, augment=augment)
        out.append(t if keep_on_device else t.cpu())
    return out


def _augment_hyp(args):
    """AugmentHyp from the cfg: every augmentation key the cfg (or a train(**kwargs) override) carries, the reference's defaults else"""
    return AugmentHyp(**{k: getattr(args, k) for k in vars(AugmentHyp()) if getattr(args, k, None) is not None})


def build_train_loader(args, data, task, device="cuda", rank=-1, world_size=1):
    """The training set of a checked data dict (dataset.check_det_dataset) as a DeviceAugmentLoader: what build_yolo_dataset(mode=
    'train') + build_dataloader are in the reference (ultralytics/data/build.py:72-109).  Labels are read and verified
    (dataset.load_split: fraction, single_cls, classes), every image is decoded once and resized on the device to its load_image size
    (linear: augment=True).  The images stay in HBM unless they would take more than half of the free device memory
    (torch.cuda.mem_get_info), then in pinned host memory (resident=False); the choice is logged.  world_size > 1: rank r takes the
    files r::world_size of the sorted list -- a plain shard, not DistributedSampler's per-epoch permutation."""
    from .dataset import LOGGER, decode_all, load_split, task_labels
    device = torch.device(device)
    files, labels, _ = load_split(data, "train", task, args)
    if world_size > 1:
        files, labels = files[max(rank, 0)::world_size], labels[max(rank, 0)::world_size]
    imgsz, workers = int(args.imgsz), getattr(args, "workers", 8)
    decoded = decode_all(files, workers)
    need = sum(3 * min(math.ceil(h * imgsz / max(h, w)), imgsz) * min(math.ceil(w * imgsz / max(h, w)), imgsz)
               for h, w in (im.shape[:2] for im in decoded))
    free = torch.cuda.mem_get_info(device)[0]
    resident = need <= free // 2
    LOGGER.info(f"train: {len(files)} images, {need / 2 ** 20:.1f} MiB at imgsz {imgsz}; {free / 2 ** 20:.0f} MiB of device memory free -> "
                f"{'resident in device memory' if resident else 'pinned host memory, uploaded per batch'}")
    images = _device_images(decoded, imgsz, device, augment=True, keep_on_device=resident)
    return DeviceAugmentLoader(images, task_labels(labels, task), imgsz, int(args.batch), hyp=_augment_hyp(args), device=device,
                               resident=resident, seed=int(getattr(args, "seed", 0) or 0), task=task, flip_idx=data.get("flip_idx"),
                               mask_ratio=int(getattr(args, "mask_ratio", 4)), overlap_mask=bool(getattr(args, "overlap_mask", True)))


def build_val_loader(args, data, task, device="cuda", split="val", batch=None, stride=32):
    """`split` of a checked data dict as a DeviceValLoader: build_yolo_dataset(mode='val') -- rect=True, pad=0.5 -- of the reference
    (ultralytics/data/build.py:72-88; models/yolo/detect/val.py:176-185).  `batch`: the cfg's unless given (the trainer gives 2 x)."""
    from .dataset import load_split
    files, labels, _ = load_split(data, split, task, args)
    return DeviceValLoader(files, labels, int(args.imgsz), int(batch or args.batch), stride=stride, pad=0.5, rect=True, task=task,
                           device=device, workers=getattr(args, "workers", 8), mask_ratio=int(getattr(args, "mask_ratio", 4)),
                           overlap_mask=bool(getattr(args, "overlap_mask", True)))


class DeviceValLoader:
    """The reference's validation dataset + dataloader (YOLODataset(augment=False, rect=True, pad=0.5) behind build_dataloader,
    shuffle off) with the pixels on the device.  `labels`: dataset.read_labels' dicts (with `shape`), `im_files` in the same order.
      * rect: dataset.set_rectangle orders the images by aspect ratio and gives every batch its own (H_b, W_b);
      * every image is decoded ONCE, uploaded and resized to its load_image size by load_resize(augment=False) -- dy_aug_resize_area_u8
        when it shrinks (cv2.INTER_AREA), linear when it grows -- and kept on the device between epochs;
      * per batch: dy_aug_letterbox to (H_b, W_b), scaleup=False, centred, border 114, CHW RGB; labels through val_labels.
    Batches follow the reference's collate schema: img uint8 [b, 3, H_b, W_b] (device), batch_idx [N], cls [N, 1], bboxes [N, 4]
    normalised xywh, im_file, ori_shape (decoded h, w), resized_shape (load_image h, w), ratio_pad = ((h / h0, w / w0), (dw, dh)) as
    get_image_and_label + LetterBox leave it (base.py:245-246, augment.py:589-590); segment adds `masks` (and cls / bboxes / batch_idx
    become the device rows in mask order), pose adds `keypoints` [N, K, 3].  The last batch may be smaller."""

    def __init__(self, im_files, labels, imgsz, batch_size, stride=32, pad=0.5, rect=True, task="detect", device="cuda", workers=8,
                 mask_ratio=4, overlap_mask=True):
        from .dataset import decode_all, set_rectangle, task_labels
        if len(im_files) != len(labels) or not labels:
            raise ValueError("DeviceValLoader: one label dict per image file, at least one")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceValLoader: the pixel pipeline only exists on the device")
        self.imgsz, self.bs, self.task = int(imgsz), int(batch_size), task
        self.mask_ratio, self.overlap_mask = int(mask_ratio), bool(overlap_mask)
        n = len(labels)
        if rect:
            order, self.batch, self.batch_shapes = set_rectangle([lab["shape"] for lab in labels], self.bs, self.imgsz, stride, pad)
        else:
            order, self.batch = np.arange(n), np.arange(n) // self.bs
            self.batch_shapes = np.full((int(self.batch[-1]) + 1, 2), self.imgsz)
        self.order = [int(i) for i in order]
        self.im_files = [im_files[i] for i in self.order]
        self.labels = task_labels([labels[i] for i in self.order], task)
        decoded = decode_all(self.im_files, workers)
        self.ori_shapes = [(int(im.shape[0]), int(im.shape[1])) for im in decoded]
        self.images = _device_images(decoded, self.imgsz, self.device, augment=False)
        self.samples = [self._sample(k) for k in range(n)]

    def __len__(self):
        return int(self.batch[-1]) + 1

    def _sample(self, k):
        """label bookkeeping of image k (position in rect order), once: (cls, bboxes, [polygons | keypoints]), ratio_pad"""
        from .augment import val_labels
        lab, im = self.labels[k], self.images[k]
        shape = (int(im.shape[0]), int(im.shape[1]))
        out = val_labels(lab["bboxes"], shape, self.imgsz, segments=lab.get("segments"), keypoints=lab.get("keypoints"),
                         rect_shape=tuple(int(v) for v in self.batch_shapes[self.batch[k]]))
        (h0, w0), geo = self.ori_shapes[k], out[2]
        meta = dict(resized_shape=shape, ratio_pad=((shape[0] / h0, shape[1] / w0), (geo.dw, geo.dh)))
        return (np.array(lab["cls"], dtype=np.float32).reshape(-1, 1), out[0]) + tuple(out[3:]), meta

    def __iter__(self):
        from .augment import collate, letterbox_batch
        for b in range(len(self)):
            ks = [k for k in range(len(self.images)) if self.batch[k] == b]
            H, W = (int(v) for v in self.batch_shapes[b])
            img, _ = letterbox_batch([self.images[k] for k in ks], (H, W), scaleup=False)
            lab = [self.samples[k][0] for k in ks]
            meta = dict(im_file=[self.im_files[k] for k in ks], ori_shape=[self.ori_shapes[k] for k in ks],
                        resized_shape=[self.samples[k][1]["resized_shape"] for k in ks],
                        ratio_pad=[self.samples[k][1]["ratio_pad"] for k in ks])
            if self.task == "segment":
                if H % self.mask_ratio or W % self.mask_ratio:
                    raise ValueError("the batch shape must be a multiple of mask_ratio")
                dev = lambda a: torch.from_numpy(a).to(self.device)
                rows = dev(pack_rows(lab))
                masks, rows_sorted, _ = polygon_masks(dev(pack_polygons(lab)), dev(instance_offsets(lab)), rows, len(lab), H, W,
                                                      self.mask_ratio, self.overlap_mask)
                rows = rows_sorted if self.overlap_mask else rows
                yield dict(img=img, batch_idx=rows[:, 0], cls=rows[:, 1:2], bboxes=rows[:, 2:6], masks=masks, **meta)
                continue
            bi, cls, bb = collate([l[:2] for l in lab])
            batch = dict(img=img, batch_idx=bi, cls=cls, bboxes=bb, **meta)
            if self.task == "pose":
                batch["keypoints"] = torch.from_numpy(np.concatenate([l[2] for l in lab], 0))
            yield batch


# ---------------------------------------------------------------------------------------------------------------- classify
class ClassifyTrainLoader:
    """Training batches of the classify task: {img: uint8 [B, 3, S, S] RGB (device), cls: int64 [B] (device)}, the schema the
    trainer's _preprocess_classify takes.  `images`: decoded uint8 HWC BGR arrays (dataset.decode), kept at their DECODED size --
    resident=True in device memory, resident=False in pinned host memory with the sources of a batch uploaded for it; `cls`: one class
    id per image.  Per batch the host plans every sample (plan_cls_sample: random resized crop, flips, RandomHSV tables -- the project's
    own augmentation, see there; augment=False: the reference's centre crop, center_crop_rect), writes the descriptors into a pinned
    ring and ONE dy_cls_render launch on the loader's stream crops, resizes, flips, recolours and transposes the whole batch; batch
    k + 1 is issued while step k runs, as in DeviceAugmentLoader.  The generators are the loader's own (seed, seed + 1)."""

    RING = 3

    def __init__(self, images, cls, imgsz, batch_size, hyp=None, device="cuda", resident=True, seed=0, shuffle=True, drop_last=True,
                 augment=True):
        from .augment import ClassifyHyp
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ClassifyTrainLoader: the pixel pipeline only exists on the device")
        self.imgsz, self.bs, self.hyp = int(imgsz), int(batch_size), hyp or ClassifyHyp()
        self.augment, self.shuffle, self.drop_last, self.resident = bool(augment), shuffle, drop_last, bool(resident)
        if len(images) != len(cls):
            raise ValueError("ClassifyTrainLoader: one class id per image")
        host = [im if torch.is_tensor(im) else torch.from_numpy(np.ascontiguousarray(im)) for im in images]
        for im in host:
            if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or not im.is_contiguous():
                raise ValueError("ClassifyTrainLoader: images must be contiguous uint8 HWC with 3 channels")
        self.shapes = [(int(im.shape[0]), int(im.shape[1])) for im in host]
        self.images = [im.to(self.device) for im in host] if self.resident else [im if im.is_cuda else im.pin_memory() for im in host]
        self.cls = torch.as_tensor(np.asarray(cls), dtype=torch.int64).reshape(-1).to(self.device)
        self.rnd = _random.Random(seed)
        self.nprnd = np.random.RandomState(seed + 1)
        self.uploaded_bytes = 0
        self._ring = None

    def __len__(self):
        n = len(self.shapes)
        return n // self.bs if self.drop_last else -(-n // self.bs)

    def _slot(self):
        import ctypes as C
        from .._C import ClsSample
        if self._ring is None:
            self._ring = [dict(desc=torch.empty(self.bs * C.sizeof(ClsSample), dtype=torch.uint8).pin_memory(),
                               idx=torch.empty(self.bs, dtype=torch.int64).pin_memory(), ev=torch.cuda.Event()) for _ in range(self.RING)]
            self._turn = 0
            self.stream = torch.cuda.Stream(device=self.device)
        slot = self._ring[self._turn % self.RING]
        self._turn += 1
        slot["ev"].synchronize()
        return slot

    def _prepare(self, indices):
        from .augment import center_plan, cls_render, plan_cls_sample
        if self.augment:
            plans = [plan_cls_sample(self.shapes[i], self.hyp, self.rnd, self.nprnd) for i in indices]
        else:
            plans = [center_plan(self.shapes[i]) for i in indices]
        slot = self._slot()
        slot["idx"][:len(indices)] = torch.as_tensor(indices, dtype=torch.int64)
        with torch.cuda.stream(self.stream):
            if self.resident:
                srcs = [self.images[i] for i in indices]
            else:
                up = {i: self.images[i].to(self.device, non_blocking=True) for i in sorted(set(indices))}
                self.uploaded_bytes += sum(t.numel() for t in up.values())
                srcs = [up[i] for i in indices]
            img = cls_render(srcs, plans, self.imgsz, staging=slot["desc"])
            cls = self.cls[slot["idx"][:len(indices)].to(self.device, non_blocking=True)]
            slot["ev"].record(self.stream)
        return dict(img=img, cls=cls), slot["ev"], (img, cls)

    def __iter__(self):
        order = list(range(len(self.shapes)))
        if self.shuffle:
            self.rnd.shuffle(order)
        chunks = [order[i:i + self.bs] for i in range(0, len(order), self.bs)]
        if self.drop_last:
            chunks = [c for c in chunks if len(c) == self.bs]
        nxt = self._prepare(chunks[0]) if chunks else None
        for k in range(len(chunks)):
            batch, ev, tensors = nxt
            cur = torch.cuda.current_stream()
            cur.wait_event(ev)
            for t in tensors:
                t.record_stream(cur)
            yield batch
            nxt = self._prepare(chunks[k + 1]) if k + 1 < len(chunks) else None


class ClassifyValLoader:
    """Validation (and test) batches of the classify task: every file is decoded once, centre-cropped and resized on the device
    (augment.center_crop_batch: the reference's classify_transforms, CenterCrop(imgsz) + ToTensor, data/augment.py:799-806) -- a batch
    per launch -- and the rendered uint8 [b, 3, S, S] batches are kept between epochs; the decoded sources are not.  File order is kept,
    the last batch may be smaller.  Batches: {img, cls int64 [b] (device), im_file}."""

    def __init__(self, files, cls, imgsz, batch_size, device="cuda", workers=8):
        from .augment import center_crop_batch
        from .dataset import decode_all
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ClassifyValLoader: the pixel pipeline only exists on the device")
        if len(files) != len(cls) or not len(files):
            raise ValueError("ClassifyValLoader: one class id per image file, at least one")
        self.imgsz, self.bs, self.im_files = int(imgsz), int(batch_size), [str(f) for f in files]
        self.cls = torch.as_tensor(np.asarray(cls), dtype=torch.int64).reshape(-1).to(self.device)
        self.ori_shapes, self.batches = [], []
        with torch.cuda.device(self.device):
            for o in range(0, len(self.im_files), self.bs):
                decoded = decode_all(self.im_files[o:o + self.bs], workers)
                self.ori_shapes += [(int(im.shape[0]), int(im.shape[1])) for im in decoded]
                self.batches.append(center_crop_batch([torch.from_numpy(im).to(self.device) for im in decoded], self.imgsz))

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for k, img in enumerate(self.batches):
            o = k * self.bs
            yield dict(img=img, cls=self.cls[o:o + len(img)], im_file=self.im_files[o:o + len(img)])


def _classify_hyp(args):
    from .augment import ClassifyHyp
    return ClassifyHyp(**{k: getattr(args, k) for k in vars(ClassifyHyp()) if getattr(args, k, None) is not None})


def build_cls_train_loader(args, data, device="cuda", rank=-1, world_size=1):
    """The training split of a check_cls_dataset dict as a ClassifyTrainLoader (the reference: ClassificationTrainer.build_dataset /
    get_dataloader, models/yolo/classify/train.py:69-85).  Files by dataset.image_folder (`fraction` applies), decoded once; kept in
    device memory unless the decoded bytes exceed half of the free device memory, then in pinned host memory -- the rule and the log
    line of build_train_loader.  world_size > 1: rank r takes the samples r::world_size."""
    from .dataset import LOGGER, decode_all, load_cls_split
    device = torch.device(device)
    files, cls = load_cls_split(data, "train", args)
    if world_size > 1:
        files, cls = files[max(rank, 0)::world_size], cls[max(rank, 0)::world_size]
    imgsz = int(args.imgsz)
    decoded = decode_all(files, getattr(args, "workers", 8))
    need = sum(im.size for im in decoded)
    free = torch.cuda.mem_get_info(device)[0]
    resident = need <= free // 2
    LOGGER.info(f"train: {len(files)} images, {need / 2 ** 20:.1f} MiB at their decoded size; {free / 2 ** 20:.0f} MiB of device memory free -> "
                f"{'resident in device memory' if resident else 'pinned host memory, uploaded per batch'}")
    loader = ClassifyTrainLoader(decoded, cls, imgsz, int(args.batch), hyp=_classify_hyp(args), device=device, resident=resident,
                                 seed=int(getattr(args, "seed", 0) or 0))
    loader.im_files = files
    return loader


def build_cls_val_loader(args, data, device="cuda", split="val", batch=None):
    """`split` ('val' or 'test'; check_cls_dataset has already let each fall back to the other) of a check_cls_dataset dict as a
    ClassifyValLoader.  `batch`: the cfg's unless given (the trainer gives 2 x, classify/train.py:100-103)."""
    from .dataset import load_cls_split
    files, cls = load_cls_split(data, split, args)
    return ClassifyValLoader(files, cls, int(args.imgsz), int(batch or args.batch), device=device, workers=getattr(args, "workers", 8))

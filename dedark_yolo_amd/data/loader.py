"""Batches of the device input pipeline for the training loop: what `build_dataloader` + the dataloader workers are in the
reference (ultralytics/data/build.py:72-109, dataset.py:171-188), with the decoded images kept in device memory.

`DeviceAugmentLoader` owns the decoded uint8 images.  `resident=True` (the MI355X-sized default: 288 GB of HBM holds a VOC-scale dataset
several times over -- 16.5 k images x ~0.9 MB) keeps them in HBM, so a step reads nothing over PCIe; `resident=False` keeps them in pinned
host memory and uploads the source images of batch i+1 on a copy stream while step i runs (the PCIe-inclusive mode bench.py reports).
Either way the augmented pixels are produced on the device by ONE launch per batch (DeviceAugmenter.render)."""
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

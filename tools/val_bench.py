#!/usr/bin/env python3
"""Cost of the validation bookkeeping: DetectionValidator.update_metrics on the device (one dy_val_box_match per batch, nothing read
back) against the per-image host loop it replaced, which this tool keeps for the comparison (`HostLoopValidator`: one `cnt.tolist()`,
one `pred.cpu()` per image, scale_boxes / box_iou / match_predictions in torch and numpy on the host).

  1. update_metrics alone on synthetic NMS outputs: B = 32 images, 300 detections and 20 labels each, nc = 80, 10 IoU thresholds.
     Timed from the call to the end of the work it queued (torch.cuda.synchronize()); the read-back of get_stats is timed separately.
  2. a whole val() of yolov8l at 640 x 640, conf = 0.001 (class biases raised so that NMS keeps max_det detections per image).

Both paths run in ONE process in rotating order (kernel, host / host, kernel / ...): 3 warm-up rounds, then the median, minimum and
maximum of 20.  Prints one JSON document and writes it to --out.

  python tools/val_bench.py --out profiles/val_match_bench.json"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dedark_yolo_amd import ops as kops  # noqa: E402
from dedark_yolo_amd.engine.trainer import get_cfg  # noqa: E402
from dedark_yolo_amd.engine.validator import DetectionValidator, match_predictions  # noqa: E402
from dedark_yolo_amd.utils import ops  # noqa: E402


class HostLoopValidator(DetectionValidator):
    """The bookkeeping as it was before dy_val_box_match: the per-image list of non_max_suppression (one cnt.tolist()), then per image a
    copy to the host, scale_boxes, box_iou and the numpy loop over the thresholds.  No confusion matrix."""

    d2h = 0

    def postprocess(self, preds, nc=0):
        a = self.args
        self.d2h += 1                                             # cnt.tolist() inside non_max_suppression
        return ops.non_max_suppression(preds, self.conf, a.iou, multi_label=True, agnostic=False, max_det=a.max_det)

    def update_metrics(self, preds, batch):
        bi = batch["batch_idx"].cpu()
        cls_all, box_all = batch["cls"].cpu().float(), batch["bboxes"].cpu().float()
        height, width = batch["img"].shape[2:]
        for si, pred in enumerate(preds):
            pred = pred.cpu()
            self.d2h += 1
            idx = bi == si
            cls, bbox = cls_all[idx], box_all[idx]
            nl, npr = cls.shape[0], pred.shape[0]
            shape = batch["ori_shape"][si] if "ori_shape" in batch else (height, width)
            ratio_pad = batch["ratio_pad"][si] if "ratio_pad" in batch else None
            correct = torch.zeros(npr, self.niou, dtype=torch.bool)
            self.seen += 1
            if npr == 0:
                if nl:
                    self._rows.append((correct, torch.zeros(0), torch.zeros(0), cls.squeeze(-1)))
                continue
            predn = pred.clone()
            ops.scale_boxes((height, width), predn[:, :4], shape, ratio_pad=ratio_pad)
            if nl:
                tbox = ops.xywh2xyxy(bbox) * torch.tensor((width, height, width, height), dtype=torch.float32)
                ops.scale_boxes((height, width), tbox, shape, ratio_pad=ratio_pad)
                correct = match_predictions(predn, torch.cat((cls, tbox), 1), self.iouv)
            self._rows.append((correct, pred[:, 4], pred[:, 5], cls.squeeze(-1)))


def summary(ms):
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), n=len(ms))


def rotate(fns, rounds, warmup):
    """fns: name -> callable returning milliseconds; every round runs all of them, the starting one rotating"""
    names = list(fns)
    out = {n: [] for n in names}
    for r in range(warmup + rounds):
        for k in range(len(names)):
            n = names[(r + k) % len(names)]
            ms = fns[n]()
            if r >= warmup:
                out[n].append(ms)
    return {n: summary(v) for n, v in out.items()}


def synthetic_batch(gen, B, n_det, n_lab, nc, S):
    lab = np.concatenate([gen.uniform(0.2, 0.8, (B, n_lab, 2)), gen.uniform(0.05, 0.3, (B, n_lab, 2))], 2)
    cls = gen.integers(0, nc, (B, n_lab))
    det = np.zeros((B, n_det, 6), dtype=np.float32)
    for b in range(B):
        i = np.arange(n_det) % n_lab
        xy, wh = lab[b, i, :2] * S, lab[b, i, 2:] * S
        det[b, :, :4] = np.concatenate([xy - wh / 2, xy + wh / 2], 1) + gen.normal(0, 3, (n_det, 4)) * (1 + np.arange(n_det)[:, None] // n_lab)
        det[b, :, 4] = np.sort(gen.uniform(0.001, 1, n_det))[::-1]
        det[b, :, 5] = np.where(gen.random(n_det) < 0.8, cls[b, i], gen.integers(0, nc, n_det))
    batch = dict(img=torch.zeros(B, 3, S, S, device="cuda"), batch_idx=torch.arange(B).repeat_interleave(n_lab).float(),
                 cls=torch.from_numpy(cls.reshape(-1, 1).astype(np.float32)), bboxes=torch.from_numpy(lab.reshape(-1, 4).astype(np.float32)),
                 ori_shape=[(S, S)] * B)
    return torch.from_numpy(det).cuda(), torch.full((B,), n_det, dtype=torch.int32, device="cuda"), batch


def bench_update_metrics(rounds, warmup):
    B, n_det, n_lab, nc, S = 32, 300, 20, 80, 640
    out, cnt, batch = synthetic_batch(np.random.default_rng(0), B, n_det, n_lab, nc, S)
    fake = type("M", (), dict(model=[type("H", (), dict(nc=nc))()], names={i: str(i) for i in range(nc)}))()
    vals = {}
    for name, V in (("kernel", DetectionValidator), ("host", HostLoopValidator)):
        v = V(get_cfg(dict(conf=0.001)))
        v.device = torch.device("cuda")
        vals[name] = v
    readback = []

    def kernel():
        v = vals["kernel"]
        v.init_metrics(fake)
        torch.cuda.synchronize()
        t = time.perf_counter()
        v.update_metrics((out, cnt), batch)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        v.get_stats()
        readback.append((time.perf_counter() - t) * 1e3)
        return ms

    def host():
        v = vals["host"]
        v.init_metrics(fake)
        torch.cuda.synchronize()
        t = time.perf_counter()
        n = cnt.tolist()                                          # what the parent's non_max_suppression did before it returned its list
        v.update_metrics([out[i, :n[i]] for i in range(B)], batch)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    res = rotate(dict(kernel=kernel, host=host), rounds, warmup)
    a = [torch.cat(x, 0) for x in zip(*vals["kernel"].stats)]
    b = [torch.cat(x, 0) for x in zip(*vals["host"].stats)]
    assert all(torch.equal(x, y.to(x.dtype)) for x, y in zip(a, b)), "the two paths disagree"
    res["kernel"]["d2h_copies_per_batch"] = 0
    res["host"]["d2h_copies_per_batch"] = 1 + B
    res["kernel_get_stats_readback"] = summary(readback[warmup:])
    res["workload"] = dict(B=B, detections=n_det, labels=n_lab, nc=nc, thresholds=10, true_positives_at_50=int(a[0][:, 0].sum()))
    return res


def bench_val(rounds, warmup, batches, B):
    from dedark_yolo_amd.nn.tasks import DetectionModel
    torch.manual_seed(0)
    nc, S = 80, 640
    model = DetectionModel("yolov8l.yaml", nc=nc).cuda().eval()
    for name, p in model.named_parameters():
        if ".cv3." in name and name.endswith("2.bias"):
            p.data += 6.0
    gen = np.random.default_rng(1)
    loader = []
    for _ in range(batches):
        lab = np.concatenate([gen.uniform(0.2, 0.8, (B * 20, 2)), gen.uniform(0.05, 0.3, (B * 20, 2))], 1).astype(np.float32)
        loader.append(dict(img=torch.from_numpy(gen.integers(0, 256, (B, 3, S, S), dtype=np.uint8)).cuda(),
                           batch_idx=torch.arange(B).repeat_interleave(20).float(), cls=torch.from_numpy(gen.integers(0, nc, (B * 20, 1)).astype(np.float32)),
                           bboxes=torch.from_numpy(lab), ori_shape=[(S, S)] * B))
    vals = dict(kernel=DetectionValidator(get_cfg(dict(conf=0.001, verbose=False))), host=HostLoopValidator(get_cfg(dict(conf=0.001, verbose=False))))
    last = {}

    def run(name):
        def f():
            torch.cuda.synchronize()
            t = time.perf_counter()
            last[name] = vals[name](model, loader)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3
        return f

    res = rotate({n: run(n) for n in vals}, rounds, warmup)
    dets = sum(len(r[1]) for r in vals["kernel"].stats) / (batches * B)
    res["workload"] = dict(model="yolov8l.yaml", imgsz=S, conf=0.001, batches=batches, B=B, detections_per_image=round(dets, 1),
                           compute_dtype=str(kops.get_compute_dtype()), metrics_equal=last["kernel"] == last["host"],
                           metrics=last["kernel"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--val-batches", type=int, default=2)
    ap.add_argument("--val-batch", type=int, default=32)
    ap.add_argument("--skip-val", action="store_true")
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), update_metrics=bench_update_metrics(a.rounds, a.warmup))
    if not a.skip_val:
        res["val"] = bench_val(a.rounds, a.warmup, a.val_batches, a.val_batch)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

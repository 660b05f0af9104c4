"""Training throughput of a segment, pose or classify model (yolov8l-seg / yolov8l-pose / yolov8l-cls by default) on synthetic
batches: bench.py's batch law plus the task's labels -- overlap index masks at the proto resolution (imgsz / 4), or 17 keypoints per
box (normalised xy around the box centre, visibility 0 / 1 / 2); for classify uint8 images and one int64 class per image (nc =
1000) -- one train_step per iteration (preprocess + forward + loss + backward + optimizer), timed with device events after a
warm-up.  Prints one JSON line.

  python tools/task_bench.py --task {segment,pose,classify} [--model yolov8l-seg.yaml | yolov8l-pose.yaml | yolov8l-cls.yaml]
                             [--imgsz 640 | 224] [--batch 32 | 128] [--dtype bf16] [--steps 10 | 15] [--warmup 3]
                             [--deterministic] [--dump-outputs DIR] [--loader]

`--deterministic` trains on the one-stream schedule (two runs of one build then give the same bits); `--dump-outputs DIR` writes
what the last timed step computed as DIR/*.npy (bench.dump_outputs), to compare two builds output for output.

`--loader` puts the device input pipeline in the loop instead of the four fixed batches: a synthetic RESIDENT dataset (96 images with
a 640-pixel long side, 10 instances each: 5..12-vertex polygons, or 17 keypoints) is fed through
DeviceAugmentLoader(task=...) -- mosaic, affine, HSV, flips, and for the segment task the polygon rasteriser -- so the step time
includes the host's label bookkeeping and the loader's kernels.  The JSON line then also carries the label rows per batch.
For classify the dataset is folder-shaped instead: 3 x batch decoded images whose sides vary between 256 and 500 pixels, one class id
each, resident, fed through ClassifyTrainLoader (random resized crop, flips, HSV tables, one dy_cls_render launch per batch).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def add_masks(b, i, B, S):
    import torch
    h = w = S // 4
    m = torch.zeros((B, h, w), dtype=torch.uint8)
    k = [0] * B
    for bi, (cx, cy, bw, bh) in zip(b["batch_idx"].long().tolist(), b["bboxes"].tolist()):
        k[bi] += 1
        m[bi, max(int((cy - bh / 2) * h), 0):int((cy + bh / 2) * h), max(int((cx - bw / 2) * w), 0):int((cx + bw / 2) * w)] = k[bi]
    b["masks"] = m.cuda()


def add_keypoints(b, i, B, S, K=17):
    import numpy as np
    import torch
    g = np.random.default_rng(200 + i)
    n = b["bboxes"].shape[0]
    wh = b["bboxes"][:, None, 2:].numpy()
    xy = b["bboxes"][:, None, :2].numpy() + g.uniform(-0.5, 0.5, (n, K, 2)) * wh
    v = g.integers(0, 3, (n, K, 1))
    b["keypoints"] = torch.from_numpy(np.concatenate([xy, v], 2).astype(np.float32))


def loader_dataset(task, n, S, per_image=10, K=17):
    """n decoded images (long side S) with `per_image` instances each: star-shaped polygons + their boxes, or boxes + K keypoints"""
    import numpy as np
    g = np.random.default_rng(300)
    ims, labels = [], []
    for i in range(n):
        h, w = (S, int(g.integers(S * 3 // 4, S + 1))) if i % 2 else (int(g.integers(S * 3 // 4, S + 1)), S)
        ims.append(g.integers(0, 256, (h, w, 3), dtype=np.uint8))
        k = per_image
        cxy = g.uniform(0.15, 0.85, (k, 2))
        lab = dict(cls=g.integers(0, 20, (k, 1)).astype(np.float32))
        if task == "segment":
            segs, boxes = [], []
            for j in range(k):
                nv = int(g.integers(5, 13))
                ang, rad = np.sort(g.uniform(0, 2 * np.pi, nv)), g.uniform(0.04, 0.15, nv)
                p = np.clip(cxy[j] + np.stack((rad * np.cos(ang), rad * np.sin(ang)), 1), 0.0, 1.0).astype(np.float32)
                segs.append(p)
                boxes.append([(p[:, 0].min() + p[:, 0].max()) / 2, (p[:, 1].min() + p[:, 1].max()) / 2, np.ptp(p[:, 0]), np.ptp(p[:, 1])])
            lab.update(segments=segs, bboxes=np.array(boxes, dtype=np.float32))
        else:
            wh = g.uniform(0.08, 0.3, (k, 2))
            kp = cxy[:, None, :] + g.uniform(-0.5, 0.5, (k, K, 2)) * wh[:, None, :]
            lab.update(bboxes=np.concatenate((cxy, wh), 1).astype(np.float32),
                       keypoints=np.concatenate((kp, g.integers(0, 3, (k, K, 1))), 2).astype(np.float32))
        labels.append(lab)
    return ims, labels


COCO_FLIP_IDX = [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]


def classify_dataset(n, nc, lo=256, hi=500):
    """n decoded images with sides in [lo, hi] (what a folder of photographs decodes to) and one class id each"""
    import numpy as np
    g = np.random.default_rng(301)
    ims = [g.integers(0, 256, (int(g.integers(lo, hi + 1)), int(g.integers(lo, hi + 1)), 3), dtype=np.uint8) for _ in range(n)]
    return ims, g.integers(0, nc, n).astype(np.int64)


def loader_batches(task, B, S, nc=None):
    """endless stream of loader batches (epoch after epoch)"""
    from dedark_yolo_amd.data import ClassifyTrainLoader, DeviceAugmentLoader
    if task == "classify":
        ims, cls = classify_dataset(3 * B, nc)
        ld = ClassifyTrainLoader(ims, cls, S, B, seed=0, resident=True)
    else:
        ims, labels = loader_dataset(task, 3 * B, S)
        ld = DeviceAugmentLoader(ims, labels, S, B, seed=0, task=task, flip_idx=COCO_FLIP_IDX if task == "pose" else None)
    while True:
        yield from ld


# task -> (default model, default timed steps, what adds the task's labels to a batch, model class in nn.tasks)
TASKS = dict(segment=("yolov8l-seg.yaml", 10, add_masks, "SegmentationModel"), pose=("yolov8l-pose.yaml", 15, add_keypoints, "PoseModel"),
             classify=("yolov8l-cls.yaml", 15, None, "ClassificationModel"))


def classify_batch(i, B, S, nc):
    """uint8 images and one class per image, resident on the device"""
    import numpy as np
    import torch
    g = np.random.default_rng(100 + i)
    return dict(img=torch.from_numpy(g.integers(0, 256, (B, 3, S, S), dtype=np.uint8)).cuda(),
                cls=torch.from_numpy(g.integers(0, nc, B).astype(np.int64)).cuda())


def main():
    import torch
    import bench
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, get_cfg
    from dedark_yolo_amd.nn import tasks
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", choices=sorted(TASKS), required=True)
    ap.add_argument("--model")
    ap.add_argument("--imgsz", type=int, help="default 640 (classify: 224)")
    ap.add_argument("--batch", type=int, help="default 32 (classify: 128)")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--steps", type=int)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--dump-outputs", metavar="DIR")
    ap.add_argument("--loader", action="store_true",
                    help="feed the steps from DeviceAugmentLoader (classify: ClassifyTrainLoader) over a synthetic resident dataset")
    a = ap.parse_args()
    model, steps, add_labels, model_cls = TASKS[a.task]
    model, steps = a.model or model, a.steps or steps
    cls_task = a.task == "classify"
    nc, S, B = (1000 if cls_task else 20), a.imgsz or (224 if cls_task else 640), a.batch or (128 if cls_task else 32)
    torch.manual_seed(0)          # the initial weights: with the seeded batches, two runs start from the same state
    tr = DetectionTrainer(get_cfg(dict(model=model, dtype=a.dtype, optimizer="SGD", batch=B, imgsz=S, deterministic=a.deterministic)))
    tr.setup(getattr(tasks, model_cls)(tasks.yaml_model_load(model), nc=nc))
    rows, host = [], []
    if a.loader:
        stream = loader_batches(a.task, B, S, nc)

        def batch(i):
            t0 = time.perf_counter()
            b = next(stream)                                  # host: plans + label bookkeeping + enqueueing the NEXT batch's uploads / kernels
            host.append(time.perf_counter() - t0)
            rows.append(int(b["cls"].shape[0]))
            return b
    else:
        batches = []
        for i in range(4):
            if cls_task:
                batches.append(classify_batch(i, B, S, nc))
                continue
            b = bench.synth_batch(100 + i, B, S, nc, "cpu")
            b.pop("gamma")
            add_labels(b, i, B, S)
            b["img"] = b["img"].cuda()
            batches.append(b)

        def batch(i):
            return batches[i % 4]
    for i in range(a.warmup):
        tr.train_step(dict(batch(i)), [0.01] * 3, 0.9)
    torch.cuda.synchronize()
    del rows[:], host[:]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        loss, items = tr.train_step(dict(batch(i)), [0.01] * 3, 0.9)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    if a.dump_outputs:
        bench.dump_outputs(a.dump_outputs, tr, loss, items)
    print(json.dumps(dict(metric=f"{a.task} training img/s", model=model, imgsz=S, batch=B, dtype=a.dtype, steps=steps,
                          warmup=a.warmup, ms_per_step=round(ms, 3), value=round(B * 1000.0 / ms, 2),
                          items=[round(float(v), 4) for v in items.reshape(-1)],
                          **(dict(loader=True, dataset_instances_per_image=1 if cls_task else 10,
                                  label_rows_per_batch=round(sum(rows) / len(rows), 1),
                                  host_loader_ms_per_step=round(1e3 * sum(host) / len(host), 3)) if a.loader else {}))))


if __name__ == "__main__":
    main()

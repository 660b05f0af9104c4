"""Training throughput of a pose model (yolov8l-pose by default) on synthetic batches: bench.py's batch law plus 17 keypoints per
box (normalised xy around the box centre, visibility 0 / 1 / 2), one train_step per iteration (preprocess + forward + detection and
keypoint loss + backward + optimizer), timed with device events after a warm-up.  Prints one JSON line.

  python tools/pose_bench.py [--model yolov8l-pose.yaml] [--imgsz 640] [--batch 32] [--dtype bf16] [--steps 15] [--warmup 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def keypoints(b, K, seed):
    import numpy as np
    import torch
    g = np.random.default_rng(seed)
    n = b["bboxes"].shape[0]
    wh = b["bboxes"][:, None, 2:].numpy()
    xy = b["bboxes"][:, None, :2].numpy() + g.uniform(-0.5, 0.5, (n, K, 2)) * wh
    v = g.integers(0, 3, (n, K, 1))
    return torch.from_numpy(np.concatenate([xy, v], 2).astype(np.float32))


def main():
    import torch
    import bench
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, get_cfg
    from dedark_yolo_amd.nn.tasks import PoseModel, yaml_model_load
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="yolov8l-pose.yaml")
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    nc, S, B = 20, a.imgsz, a.batch
    tr = DetectionTrainer(get_cfg(dict(model=a.model, dtype=a.dtype, optimizer="SGD", batch=B, imgsz=S, deterministic=False)))
    tr.setup(PoseModel(yaml_model_load(a.model), nc=nc))
    batches = []
    for i in range(4):
        b = bench.synth_batch(100 + i, B, S, nc, "cpu")
        b.pop("gamma")
        b["keypoints"] = keypoints(b, 17, 200 + i)
        b["img"] = b["img"].cuda()
        batches.append(b)
    for i in range(a.warmup):
        tr.train_step(dict(batches[i % 4]), [0.01] * 3, 0.9)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(a.steps):
        loss, items = tr.train_step(dict(batches[i % 4]), [0.01] * 3, 0.9)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    print(json.dumps(dict(metric="pose training img/s", model=a.model, imgsz=S, batch=B, dtype=a.dtype, steps=a.steps,
                          warmup=a.warmup, ms_per_step=round(ms, 3), value=round(B * 1000.0 / ms, 2),
                          items=[round(float(v), 4) for v in items])))


if __name__ == "__main__":
    main()

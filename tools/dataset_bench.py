#!/usr/bin/env python3
"""Dataset-layer micro-benchmark: prints one JSON line and writes it to profiles/dataset_bench.json.

  (a) dy_aug_resize_area_u8 beside dy_aug_resize_u8 on the same source / destination shapes (960x1280 -> 480x640, exact 2:1;
      1000x1333 -> 481x640; 375x500 -> 240x320): ms and bytes/s, bytes = source + destination;
  (b) a DeviceValLoader over a synthetic set written to a temporary directory: decode time (host, thread pool) and the device time of
      the load_image resizes and of one pass over the rect batches, separately;
  (c) val() of yolov8l at 640, batch 32, from that loader, beside the same batches pre-built and passed as loader=.
Device events around every timed region; median of --reps (20) after --warmup (3), min and max beside every median.

    python tools/dataset_bench.py [--images 256] [--reps 20] [--warmup 3] [--model yolov8l.yaml] [--skip-val]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

RESIZE_SHAPES = [((960, 1280), (480, 640)), ((1000, 1333), (481, 640)), ((375, 500), (240, 320))]


def timed(fn, reps, warmup):
    """device milliseconds of fn(): dict(median, min, max) over `reps` runs after `warmup`"""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def bench_resize(reps, warmup):
    from dedark_yolo_amd._C import call
    from dedark_yolo_amd.ops import ptr, stream
    g, out = np.random.default_rng(0), []
    for (sh, sw), (dh, dw) in RESIZE_SHAPES:
        src = torch.from_numpy(g.integers(0, 256, (sh, sw, 3), dtype=np.uint8)).cuda()
        dst = torch.empty((dh, dw, 3), dtype=torch.uint8, device="cuda")
        nbytes = src.numel() + dst.numel()
        row = dict(src=[sh, sw], dst=[dh, dw], bytes=nbytes)
        for key, name in (("area", "dy_aug_resize_area_u8"), ("linear", "dy_aug_resize_u8")):
            t = timed(lambda: call(name, ptr(src), sh, sw, src.stride(0), ptr(dst), dh, dw, dst.stride(0), stream()), reps, warmup)
            t["bytes_per_s"] = nbytes / (t["median_ms"] * 1e-3)
            row[key] = t
        row["area_over_linear_bytes_per_s"] = row["area"]["bytes_per_s"] / row["linear"]["bytes_per_s"]
        out.append(row)
    return out


def write_synthetic_set(root, n, seed=0):
    """n lossless PNGs of 375..500 x 500..667 seeded pixels (a few portrait) with 1-4 boxes each, YOLO layout"""
    from PIL import Image
    g = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "images", "val"))
    os.makedirs(os.path.join(root, "labels", "val"))
    for i in range(n):
        h, w = int(g.integers(375, 501)), int(g.integers(500, 668))
        if i % 5 == 4:
            h, w = w, h
        Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(os.path.join(root, "images", "val", f"{i:04d}.png"),
                                                                                   compress_level=1)
        k = int(g.integers(1, 5))
        rows = np.concatenate((g.integers(0, 20, (k, 1)).astype(float), g.uniform(0.3, 0.7, (k, 2)), g.uniform(0.05, 0.4, (k, 2))), 1)
        with open(os.path.join(root, "labels", "val", f"{i:04d}.txt"), "w") as f:
            for r in rows:
                f.write(f"{int(r[0])} " + " ".join(f"{v:.6f}" for v in r[1:]) + "\n")
    with open(os.path.join(root, "data.yaml"), "w") as f:
        f.write("path: .\ntrain: images/val\nval: images/val\nnc: 80\n")
    return os.path.join(root, "data.yaml")


def bench_loader(yaml_path, imgsz, batch, workers, reps, warmup):
    from dedark_yolo_amd.data import DeviceValLoader, check_det_dataset
    from dedark_yolo_amd.data import dataset as ds
    from dedark_yolo_amd.data.loader import _device_images
    data = check_det_dataset(yaml_path)
    files = ds.get_img_files(data["val"])
    labels, _ = ds.read_labels(files, "detect", data["nc"], None, workers)
    wall = []
    for _ in range(3):
        t0 = time.perf_counter()
        decoded = ds.decode_all(files, workers)
        wall.append((time.perf_counter() - t0) * 1e3)
    out = dict(images=len(files), imgsz=imgsz, batch=batch, threads=ds.pool_size(workers),
               decode=dict(median_ms=statistics.median(wall), min_ms=min(wall), max_ms=max(wall), runs=3, clock="host"),
               decoded_bytes=int(sum(im.nbytes for im in decoded)))
    out["load_resize"] = timed(lambda: _device_images(decoded, imgsz, torch.device("cuda"), augment=False), reps, warmup)
    loader = DeviceValLoader(files, labels, imgsz, batch, stride=32, pad=0.5, rect=True, workers=workers)

    def one_pass():
        for _ in loader:
            pass
    out["one_pass"] = timed(one_pass, reps, warmup)
    out["batches"] = len(loader)
    return out, loader


def bench_val(loader, model_yaml, imgsz, batch, reps, warmup):
    from dedark_yolo_amd.engine.model import YOLO
    from dedark_yolo_amd.engine.trainer import get_cfg
    from dedark_yolo_amd.nn.tasks import all_tasks
    y = YOLO(model_yaml)
    y.model.cuda()
    prebuilt = list(loader)
    validator = all_tasks()[y.task][2]
    out = dict(model=model_yaml, imgsz=imgsz, batch=batch, images=len(loader.im_files))
    for key, src in (("from_loader", loader), ("prebuilt_loader_arg", prebuilt)):
        out[key] = timed(lambda: validator(get_cfg(dict(imgsz=imgsz, batch=batch)))(y.model, src), reps, warmup)
    out["from_loader_over_prebuilt"] = out["from_loader"]["median_ms"] / out["prebuilt_loader_arg"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--model", default="yolov8l.yaml")
    ap.add_argument("--skip-val", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "dataset_bench needs a GPU"
    res = dict(tool="dataset_bench", device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup)
    res["resize"] = bench_resize(a.reps, a.warmup)
    with tempfile.TemporaryDirectory() as root:
        yaml_path = write_synthetic_set(root, a.images)
        res["val_loader"], loader = bench_loader(yaml_path, a.imgsz, a.batch, a.workers, a.reps, a.warmup)
        if not a.skip_val:
            res["val"] = bench_val(loader, a.model, a.imgsz, a.batch, a.reps, a.warmup)
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "dataset_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

"""Cost of MixUp in the device input pipeline.  One JSON line.

  python tools/mixup_bench.py [--legs kernel,host,step] [--imgsz 640] [--batch 64] [--steps 20] [--warmup 3] [--out FILE]

kernel: one render launch (descriptors already on the device) for `--batch` plans over a resident synthetic dataset, device events,
  median (and minimum) of `--steps` after `--warmup`, all three legs in one process on the same images: (a) dy_aug_mosaic_warp, (b) dy_aug_mosaic_warp_mix with no sample mixed
  (the SAME plans as (a); the outputs are compared), (c) dy_aug_mosaic_warp_mix with every sample mixed.  Expectation from the code:
  (b) = (a), (c) < 2 x (a) -- the gathered taps double, the HSV conversion and the store do not.
host: the host label work (plans + train_labels) per 32-sample batch for detect / segment / pose, with mixup 0 and 1 (every sample
  mixed: the upper end; at mixup = p the cost lies p of the way between); needs no GPU.
step: yolov8l detect training steps (bf16, batch 32, 640 x 640) fed from DeviceAugmentLoader with mixup 0 and 0.15, ms per step with
  the loader in the loop.
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def detect_view(labels):
    return [dict(cls=l["cls"], bboxes=l["bboxes"]) for l in labels]


def kernel_legs(S, B, steps, warmup):
    import numpy as np
    import torch
    from dedark_yolo_amd._C import call
    from dedark_yolo_amd.data import AugmentHyp, DeviceAugmenter
    from dedark_yolo_amd.data.augment import descriptor_bytes, fill_descriptors
    from dedark_yolo_amd.ops import ptr, stream
    from task_bench import loader_dataset
    ims, labels = loader_dataset("pose", 96, S)
    labels = detect_view(labels)
    plain, mixed = DeviceAugmenter(ims, labels, S, AugmentHyp()), DeviceAugmenter(ims, labels, S, AugmentHyp(mixup=1.0))
    mixed.images = plain.images                               # one resident copy of the dataset
    mk = lambda aug: [aug.plan(i % len(ims), random.Random(i), np.random.RandomState(i)) for i in range(B)]
    p_plain, p_mixed = mk(plain), mk(mixed)
    assert all(p.mix is None for p in p_plain) and all(p.mix is not None for p in p_mixed)
    same = bool(torch.equal(plain.render(p_plain), mixed.render(p_plain)))
    out = dict(imgsz=S, batch=B, steps=steps, warmup=warmup, unmixed_outputs_equal=same)
    img = torch.empty((B, 3, S, S), dtype=torch.uint8, device="cuda")
    for name, mix, plans in (("a_plain_entry", False, p_plain), ("b_mix_entry_none_mixed", True, p_plain), ("c_mix_entry_all_mixed", True, p_mixed)):
        host = torch.zeros(B * descriptor_bytes(mix), dtype=torch.uint8)
        fill_descriptors(plans, plain.images, host.data_ptr(), mix)
        desc = host.cuda()                                    # the launch alone is timed: descriptors already on the device
        entry = "dy_aug_mosaic_warp_mix" if mix else "dy_aug_mosaic_warp"
        run = lambda: call(entry, ptr(desc), B, S, S, ptr(img), stream())
        for _ in range(warmup):
            run()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        for e0, e1 in ev:
            e0.record()
            run()
            e1.record()
        torch.cuda.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        out[name + "_ms"] = dict(median=round(ms[len(ms) // 2], 4), min=round(ms[0], 4))
    a = out["a_plain_entry_ms"]["median"]
    out["b_over_a"], out["c_over_a"] = round(out["b_mix_entry_none_mixed_ms"]["median"] / a, 3), round(out["c_mix_entry_all_mixed_ms"]["median"] / a, 3)
    return out


def host_legs(S, B=32, reps=3):
    import numpy as np
    from dedark_yolo_amd.data import augment as A
    from task_bench import COCO_FLIP_IDX, loader_dataset
    out = {}
    for task in ("detect", "segment", "pose"):
        ims, labels = loader_dataset("segment" if task == "segment" else "pose", 3 * B, S)
        shapes = [im.shape[:2] for im in ims]
        if task == "detect":
            labels = detect_view(labels)
        for mixup in (0.0, 1.0):
            ex = A.TaskLabels(labels, task, A.AugmentHyp(mixup=mixup), COCO_FLIP_IDX if task == "pose" else None, 4, True, S)
            rnd, nprnd, best, rows = random.Random(1), np.random.RandomState(2), None, 0
            for r in range(reps):
                t0 = time.perf_counter()
                plans = [A.plan_train_sample(i, shapes, list(range(len(ims))), S, ex.hyp, rnd, nprnd) for i in range(r * B, (r + 1) * B)]
                lab = [ex.train_labels(p, shapes) for p in plans]
                dt = time.perf_counter() - t0
                best, rows = (dt if best is None else min(best, dt)), sum(len(l[0]) for l in lab)
            out[f"{task}_mixup_{mixup:g}"] = dict(ms_per_batch=round(1e3 * best, 2), label_rows=rows)
    return dict(batch=B, imgsz=S, instances_per_image=10, best_of=reps, **out)


def step_legs(S=640, B=32, steps=10, warmup=3):
    import torch
    from dedark_yolo_amd.data import AugmentHyp, DeviceAugmentLoader
    from dedark_yolo_amd.engine.trainer import DetectionTrainer, get_cfg
    from dedark_yolo_amd.nn import tasks
    from task_bench import loader_dataset
    ims, labels = loader_dataset("pose", 3 * B, S)
    labels = detect_view(labels)
    torch.manual_seed(0)
    tr = DetectionTrainer(get_cfg(dict(model="yolov8l.yaml", dtype="bf16", optimizer="SGD", batch=B, imgsz=S, deterministic=False)))
    tr.setup(tasks.DetectionModel(tasks.yaml_model_load("yolov8l.yaml"), nc=20))
    out = dict(model="yolov8l.yaml", imgsz=S, batch=B, steps=steps, warmup=warmup)
    for mixup in (0.0, 0.15, 0.0):                            # the un-mixed leg twice: its spread is the noise floor
        ld = DeviceAugmentLoader(ims, labels, S, B, hyp=AugmentHyp(mixup=mixup), seed=0)

        def stream():
            while True:
                yield from ld
        it = stream()
        for _ in range(warmup):
            tr.train_step(dict(next(it)), [0.01] * 3, 0.9)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            tr.train_step(dict(next(it)), [0.01] * 3, 0.9)
        e1.record()
        torch.cuda.synchronize()
        out.setdefault(f"mixup_{mixup:g}_ms_per_step", []).append(round(e0.elapsed_time(e1) / steps, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="kernel,host")
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    legs = a.legs.split(",")
    res = {}
    if "kernel" in legs:
        res["kernel"] = kernel_legs(a.imgsz, a.batch, a.steps, a.warmup)
    if "host" in legs:
        res["host_labels"] = host_legs(a.imgsz)
    if "step" in legs:
        res["train_step"] = step_legs()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

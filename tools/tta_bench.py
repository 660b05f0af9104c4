"""Time of augmented inference (predict(augment=True)) for detection models: per model the eval forward (a) single-scale, (b) augmented
(three passes; dy_tta_scale_img prepares two of the images, dy_detect_decode_tta writes every pass's boxes de-scaled, de-flipped and
clipped into the merged output) and (c), on the same device and in the same process, the reference's composition restated with torch
operators (flip, F.interpolate, F.pad, an in-place divide, split, subtract, two cats and two slices) around three single-scale
forwards of the same model.  Device-event timing after a warm-up, median of the timed runs; one JSON line.

  python tools/tta_bench.py [--models yolov8l.yaml,yolov8l-p2.yaml] [--imgsz 640] [--batch 32] [--dtype bf16] [--steps 20] [--warmup 3]
                            [--legs single,augment,torch]

`--legs augment` runs (b) alone: under `rocprofv3 --kernel-trace --stats` the trace then holds the augmented path's kernels only.

`expected_ratio` is the pixel count of the three passes over that of one (1 + (544 / 640)^2 + (448 / 640)^2 = 2.21 at 640): what (b)/(a)
would be if a pass cost in proportion to its pixels.  The bytes dy_tta_scale_img moves per call (source read once + output written) are
reported for use with a kernel trace.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scale_img_torch(x, ratio, gs, flip):
    import torch.nn.functional as F
    if flip:
        x = x.flip(flip)
    if ratio == 1.0:
        return x
    h, w = x.shape[2:]
    s = (int(h * ratio), int(w * ratio))
    x = F.interpolate(x, size=s, mode="bilinear", align_corners=False)
    hp, wp = (math.ceil(v * ratio / gs) * gs for v in (h, w))
    return F.pad(x, [0, wp - s[1], 0, hp - s[0]], value=0.447)


def composed(model, x, scales, flips):
    import torch
    head = model.model[-1]
    H, W = x.shape[2:]
    gs = int(max(head.strides_as_floats()))
    ys = []
    for s, f in zip(scales, flips):
        yi = model._predict_once(scale_img_torch(x, s, gs, f))[0]
        yi[:, :4] /= s
        bx, by, wh, cls = yi.split((1, 1, 2, yi.shape[1] - 4), 1)
        if f == 2:
            by = H - by
        elif f == 3:
            bx = W - bx
        ys.append(torch.cat((bx, by, wh, cls), 1))
    g = sum(4 ** k for k in range(head.nl))
    ys[0] = ys[0][..., :-(ys[0].shape[-1] // g)]
    ys[-1] = ys[-1][..., (ys[-1].shape[-1] // g) * 4 ** (head.nl - 1):]
    return torch.cat(ys, -1)


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2], ms[0]


def main():
    import numpy as np
    import torch
    import dedark_yolo_amd as dy
    from dedark_yolo_amd.nn.tasks import TTA, DetectionModel, tta_plan
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="yolov8l.yaml,yolov8l-p2.yaml")
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="single,augment,torch")
    a = ap.parse_args()
    legs = a.legs.split(",")
    if not torch.cuda.is_available():
        raise SystemExit("tta_bench needs a GPU (there is no CPU path)")
    dy.set_compute_dtype(dict(bf16=torch.bfloat16, f16=torch.float16, f32=torch.float32)[a.dtype])
    S, B = a.imgsz, a.batch
    x = torch.from_numpy(np.random.default_rng(0).random((B, 3, S, S), dtype=np.float32)).cuda()
    out = dict(tool="tta_bench", imgsz=S, batch=B, dtype=a.dtype, steps=a.steps, warmup=a.warmup, models={})
    for name in a.models.split(","):
        torch.manual_seed(0)
        model = DetectionModel(name, nc=80).cuda().eval()
        model.fuse(verbose=False)
        head = model.model[-1]
        passes, a_total = tta_plan(S, S, head.strides_as_floats(), head.nl)
        with torch.no_grad():
            single = lambda: model(x)                                             # noqa: E731
            augmented = lambda: model(x, augment=True)                            # noqa: E731
            torch_side = lambda: composed(model, x, TTA["scales"], TTA["flips"])  # noqa: E731
            r = dict(merged_anchors=a_total, pass_sizes=[[p[4], p[5]] for p in passes])
            if "augment" in legs and "torch" in legs:
                got, want = augmented()[0], torch_side()
                r["max_abs_diff_over_max_abs"] = float((got - want).abs().max()) / float(want.abs().max())
                del got, want
            for leg, fn in (("single", single), ("augment", augmented), ("torch_composition", torch_side)):
                if leg.split("_")[0] in legs:
                    med, lo = timed(fn, a.steps, a.warmup)
                    r[leg + "_ms"], r[leg + "_min_ms"] = round(med, 3), round(lo, 3)
        pixels = [p[4] * p[5] for p in passes]
        if "single_ms" in r and "augment_ms" in r:
            r["augment_over_single"] = round(r["augment_ms"] / r["single_ms"], 3)
        if "torch_composition_ms" in r and "augment_ms" in r:
            r["augment_over_torch_composition"] = round(r["augment_ms"] / r["torch_composition_ms"], 3)
        r["expected_ratio"] = round(sum(pixels) / pixels[0], 3)
        r["scale_img_bytes_per_call"] = [4 * B * 3 * (S * S + p[4] * p[5]) for p in passes[1:]]
        out["models"][name] = r
        del model
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Mask post-processing time of segment inference at image resolution on synthetic NMS outputs: yolov8l-seg's proto geometry
(32 x imgsz/4 x imgsz/4 per image, NHWC), a fixed number of detections per image with random boxes and coefficients, the three
image-resolution modes of `process_masks_batched` (one dy_seg_mask_upsample launch each) and, beside each on the same device and
in the same process, the reference's formula restated with torch operators (matmul -> sigmoid -> crop -> F.interpolate -> crop ->
> 0.5, image by image as the reference's predictor and validator loop does).  Device-event timing after a warm-up; one JSON line.

  python tools/seg_predict_bench.py [--dets 100] [--imgsz 640] [--batch 32] [--dtype bf16] [--orig 480x640] [--steps 20] [--warmup 3]

`--orig HxW` is the original image shape of the native mode (every image the same, so it is one launch as well).  The torch side
gets the proto as f32 NCHW, converted outside the timed region, so it is not charged for the layout the product keeps.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def crop(m, b):
    import torch
    h, w = m.shape[1:]
    r = torch.arange(w, device=m.device, dtype=torch.float32)[None, None, :]
    c = torch.arange(h, device=m.device, dtype=torch.float32)[None, :, None]
    x1, y1, x2, y2 = torch.chunk(b[:, :, None], 4, 1)
    return m * ((r >= x1) * (r < x2) * (c >= y1) * (c < y2))


def torch_masks(mode, proto, det, shape, out_shape, window):
    """one image: proto f32 [32, mh, mw], det [n, 38] -> f32 0 / 1 [n, h, w]"""
    import torch.nn.functional as F
    c, mh, mw = proto.shape
    m = (det[:, 6:] @ proto.view(c, -1)).sigmoid().view(-1, mh, mw)
    b = det[:, :4]
    if mode == "input":
        s = b.new_tensor([mw / shape[1], mh / shape[0], mw / shape[1], mh / shape[0]])
        return F.interpolate(crop(m, b * s)[None], shape, mode="bilinear", align_corners=False)[0].gt_(0.5)
    if mode == "native":
        top, left, bottom, right = window
        m = m[:, top:bottom, left:right]
    return crop(F.interpolate(m[None], out_shape, mode="bilinear", align_corners=False)[0], b).gt_(0.5)


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
    from dedark_yolo_amd.utils import ops as uops
    ap = argparse.ArgumentParser()
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--orig", default="480x640")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dtype = dict(bf16=torch.bfloat16, f16=torch.float16, f32=torch.float32)[a.dtype]
    S, B, n = a.imgsz, a.batch, a.dets
    orig = tuple(int(v) for v in a.orig.split("x"))
    gen = np.random.default_rng(0)
    mh = mw = S // 4
    proto32 = torch.from_numpy(gen.normal(0, 1, (B, 32, mh, mw)).astype(np.float32)).cuda()
    proto = proto32.to(dtype).contiguous(memory_format=torch.channels_last)
    proto32 = proto.float().contiguous()                                  # the same rounded values, f32 NCHW, for the torch side
    out = dict(tool="seg_predict_bench", imgsz=S, batch=B, dets_per_image=n, dtype=a.dtype, orig=list(orig), steps=a.steps)
    for mode in ("input", "upsample", "native"):
        H, W = orig if mode == "native" else (S, S)
        xy = gen.uniform(0, 0.8, (B, n, 2)) * (W, H)
        wh = gen.uniform(0.05, 0.4, (B, n, 2)) * (W, H)
        rows = np.concatenate([xy, xy + wh, gen.uniform(0.3, 1, (B, n, 1)), gen.integers(0, 80, (B, n, 1)), gen.normal(0, 0.6, (B, n, 32))], 2)
        dets = [torch.from_numpy(rows[i].astype(np.float32)).cuda() for i in range(B)]
        shapes = [(H, W)] * B
        window = uops.scale_masks_window(mh, mw, (H, W))
        fused = lambda: uops.process_masks_batched(proto, dets, (S, S), mode=mode, out_shapes=shapes)          # noqa: E731
        composed = lambda: [torch_masks(mode, proto32[i], dets[i], (S, S), (H, W), window) for i in range(B)]  # noqa: E731
        got, want = fused(), composed()
        diff = sum(int((g.bool() != w.bool()).sum()) for g, w in zip(got, want))
        f_med, f_min = timed(fused, a.steps, a.warmup)
        del got, want
        t_med, t_min = timed(composed, a.steps, a.warmup)
        out[mode] = dict(out_shape=[H, W], fused_ms=round(f_med, 3), fused_min_ms=round(f_min, 3), torch_ms=round(t_med, 3),
                         torch_min_ms=round(t_min, 3), speedup=round(t_med / f_med, 2), differing_pixels=diff,
                         pixels=B * n * H * W, out_gb_per_s=round(B * n * H * W / f_med / 1e6, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""PConv micro-benchmark: the fused kernels (dy_pconv_fwd / dgrad / wgrad) against the composite forward route -- the existing conv on
the channel slice x[:, :c3] plus dy_copy2d of the other channels (only possible where c3 is a vector multiple).  Shapes: the PConv
layers of yolov8l-Faster-2.0 at B=64, 640x640 (C = 4*c3 channels).  Prints one JSON line per shape and direction: microseconds per
call and the fraction of HBM peak the minimum traffic of the call would need at that time.

    python tools/pconv_bench.py [--dtype bf16] [--iters 50] [--peak-tbs 8.0]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(16, 160), (32, 80), (64, 40), (64, 20)]       # (c3, H = W) of yolov8l-Faster-2.0 at 640x640


def timed(fn, iters):
    import torch
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    import torch
    import dedark_yolo_amd as dy
    from dedark_yolo_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="HBM peak in TB/s for the fraction column")
    a = ap.parse_args()
    dt = dict(fp32=torch.float32, bf16=torch.bfloat16, fp16=torch.float16)[a.dtype]
    dy.set_compute_dtype(dt)
    es = torch.tensor([], dtype=dt).element_size()
    B = a.batch
    for c3, hw in SHAPES:
        C = 4 * c3
        g = torch.Generator(device="cuda").manual_seed(c3)
        x = (torch.rand((B, hw, hw, C), device="cuda", generator=g) * 2 - 1).to(dt).permute(0, 3, 1, 2)
        gy = (torch.rand((B, hw, hw, C), device="cuda", generator=g) * 2 - 1).to(dt).permute(0, 3, 1, 2)
        y = torch.empty_like(x)
        w = torch.nn.Parameter((torch.rand((c3, c3, 3, 3), device="cuda", generator=g) - 0.5) / c3)
        px = B * hw * hw
        rows = []

        def fused_fwd():
            ops.pconv_forward(None, x, w, out=y)

        def composite_fwd():
            ops.conv_forward(None, x[:, :c3], w, None, None, ops.ACT_NONE, 1, 1, 1, False, out=y[:, :c3])
            ops.copy2d(x[:, c3:], y[:, c3:])

        def fused_bwd():
            from dedark_yolo_amd.nn.modules import Tape
            t = Tape()
            t.push((x, w))
            ops.pconv_backward(t, gy, dx_out=y)

        rows.append(("fwd fused", timed(fused_fwd, a.iters), 2 * px * C * es))
        if c3 % ops.vec_elems(dt) == 0:
            rows.append(("fwd composite (conv on slice + copy2d)", timed(composite_fwd, a.iters), 2 * px * C * es))
        rows.append(("bwd fused (wgrad + dgrad)", timed(fused_bwd, a.iters), (2 * px * c3 + 2 * px * C) * es))
        for what, us, nbytes in rows:
            print(json.dumps(dict(shape=f"c3={c3} C={C} {B}x{hw}x{hw}", dtype=a.dtype, kind=what, us=round(us, 1),
                                  hbm_frac=round(nbytes / (us * 1e-6) / (a.peak_tbs * 1e12), 3))), flush=True)


if __name__ == "__main__":
    main()

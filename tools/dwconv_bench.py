#!/usr/bin/env python3
"""Depthwise-convolution micro-benchmark: dy_dwconv_fwd (epilogue and statistics mode), dy_dwconv_dgrad and dy_dwconv_wgrad on the
depthwise layers of yolov8n-ghost and yolov8l-ghost at 640x640, B = 32, bf16 -- the 5x5 stride-1 layer of the widest and of the
highest-resolution stage of each graph (plus the 4-channel half of scale n, the 8-byte aligned case) and one 3x3 stride-2 shape.
Beside every leg:
  (a) dy_copy2d moving the same number of bytes: the project's own achieved-bandwidth yardstick; its spread over the run is the noise
      floor for any claim;
  (b) torch's grouped convolution (channels-last, the same tensors): what a user would otherwise get.  A shape torch's backend refuses
      is recorded as refused; nothing falls back.
One process, device events, legs interleaved, median of --iters after --warmup.  Bytes are computed from the shapes: every leg reads
or writes pixels_in * C + pixels_out * C elements (the forward moves pixels * C * (1 / s^2 + 1)); weights are noise.  Bound per shape,
from arithmetic and not from measurement: 3x3 is 9 FMA per output, far under the vector rate at HBM speed -> HBM; 5x5 in 16-bit is 25
FMA per 4 bytes, at 6.3 TB/s about 79 TFLOP/s of f32 vector work, half the 157 TFLOP/s vector peak before the 16-bit -> f32
conversions -> near the ridge (HBM and VALU both matter).

    python tools/dwconv_bench.py [--out profiles/dwconv_bench.json] [--step NAME=bench_line.json ...]
    python tools/dwconv_bench.py --dry-run        # no GPU: shapes and byte accounting only
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (graph, layer, C, H = W of the input, k, stride)
SHAPES = [("yolov8n-ghost", "model.1.cv2 (highest resolution)", 16, 160, 5, 1),
          ("yolov8n-ghost", "model.2.m.0.conv.0.cv2 (4-channel half)", 4, 160, 5, 1),
          ("yolov8n-ghost", "model.7.cv2 (widest)", 128, 20, 5, 1),
          ("yolov8l-ghost", "model.1.cv2 (highest resolution)", 64, 160, 5, 1),
          ("yolov8l-ghost", "model.7.cv2 (widest)", 256, 20, 5, 1),
          ("3x3 stride 2", "DWConv(64, 64, 3, 2)", 64, 160, 3, 2)]


def accounting(B, C, hw, k, s, es):
    ho = (hw + 2 * (k // 2) - k) // s + 1
    pin, pout = B * hw * hw, B * ho * ho
    nbytes = (pin + pout) * C * es
    return dict(pixels_in=pin, pixels_out=pout, bytes=nbytes, flops=2 * pout * C * k * k,
                flop_per_byte=round(2 * pout * C * k * k / nbytes, 2),
                bound="HBM" if k == 3 else "near the ridge: HBM and f32 VALU (25 FMA per 4 bytes)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the result JSON here (default: print it)")
    ap.add_argument("--step", action="append", default=[], metavar="NAME=FILE", help="merge a bench.py result line as a whole-step figure")
    ap.add_argument("--dry-run", action="store_true", help="no GPU: shapes and byte accounting; every time is 'not measured'")
    a = ap.parse_args()
    es = 4 if a.dtype == "fp32" else 2
    res = dict(dtype=a.dtype, batch=a.batch, iters=a.iters, warmup=a.warmup, shapes=[], step={})
    for name_file in a.step:
        name, path = name_file.split("=", 1)
        with open(path) as f:
            lines = [ln for ln in f.read().splitlines() if ln.startswith("{")]
        res["step"][name] = json.loads(lines[-1]) if lines else "not measured"
    if a.dry_run:
        for graph, layer, C, hw, k, s in SHAPES:
            res["shapes"].append(dict(graph=graph, layer=layer, C=C, hw=hw, k=k, stride=s, **accounting(a.batch, C, hw, k, s, es),
                                      legs="not measured"))
        print(json.dumps(res, indent=1))
        return

    import torch
    import torch.nn.functional as F
    from dedark_yolo_amd import _C, ops
    dt = dict(fp32=torch.float32, bf16=torch.bfloat16, fp16=torch.float16)[a.dtype]
    did, B = ops.dt_id(dt), a.batch
    res["device"] = torch.cuda.get_device_name(0)
    scratch = torch.empty(8 << 20, dtype=torch.float32, device="cuda")

    for graph, layer, C, hw, k, s in SHAPES:
        acc = accounting(B, C, hw, k, s, es)
        ho, pad = (hw + 2 * (k // 2) - k) // s + 1, k // 2
        g = torch.Generator(device="cuda").manual_seed(C + hw)
        x = (torch.rand((B, hw, hw, C), device="cuda", generator=g) * 2 - 1).to(dt).permute(0, 3, 1, 2)
        dz = (torch.rand((B, ho, ho, C), device="cuda", generator=g) * 2 - 1).to(dt).permute(0, 3, 1, 2)
        y, dx = torch.empty_like(dz), torch.empty_like(x)
        w = ((torch.rand((C, 1, k, k), device="cuda", generator=g) - 0.5) / k).contiguous()
        dw = torch.empty_like(w)
        scale, shift = torch.rand(C, device="cuda") + 0.5, torch.rand(C, device="cuda") - 0.5
        stats = torch.zeros(64 * 2 * C, dtype=torch.float64, device="cuda")
        wt = w.to(dt).contiguous(memory_format=torch.channels_last)
        # (a): dy_copy2d of the same number of bytes: n pixels of cw channels read and written once each
        cw = max(C, 8)
        n_copy = acc["bytes"] // (2 * cw * es)
        src, dst = torch.empty((n_copy, cw), dtype=dt, device="cuda").normal_(), torch.empty((n_copy, cw), dtype=dt, device="cuda")
        st = ops.stream()
        legs = {
            "fwd_epilogue": lambda: _C.call("dy_dwconv_fwd", x.data_ptr(), C, y.data_ptr(), C, w.data_ptr(), B, hw, hw, C, k, s, scale.data_ptr(),
                                           shift.data_ptr(), 1, None, 0, did, st),
            "fwd_stats": lambda: _C.call("dy_dwconv_fwd", x.data_ptr(), C, y.data_ptr(), C, w.data_ptr(), B, hw, hw, C, k, s, None, None, 0,
                                        stats.data_ptr(), C, did, st),
            "dgrad": lambda: _C.call("dy_dwconv_dgrad", dz.data_ptr(), C, dx.data_ptr(), C, w.data_ptr(), B, hw, hw, C, k, s, 0, None, 0, did, st),
            "wgrad": lambda: _C.call("dy_dwconv_wgrad", x.data_ptr(), C, dz.data_ptr(), C, dw.data_ptr(), B, hw, hw, C, k, s, scratch.data_ptr(),
                                    scratch.numel(), did, st),
            "copy2d": lambda: _C.call("dy_copy2d", src.data_ptr(), cw, dst.data_ptr(), cw, n_copy, cw, 0, did, st),
            "torch_fwd": lambda: F.conv2d(x, wt, None, s, pad, 1, C),
            "torch_dgrad": lambda: torch.ops.aten.convolution_backward(dz, x, wt, None, [s, s], [pad, pad], [1, 1], False, [0, 0], C,
                                                                       [True, False, False]),
            "torch_wgrad": lambda: torch.ops.aten.convolution_backward(dz, x, wt, None, [s, s], [pad, pad], [1, 1], False, [0, 0], C,
                                                                       [False, True, False]),
        }
        times, refused = {n: [] for n in legs}, {}
        for it in range(a.warmup + a.iters):
            for n, fn in legs.items():
                if n in refused:
                    continue
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                try:
                    e0.record()
                    fn()
                    e1.record()
                except RuntimeError as ex:
                    if not n.startswith("torch_"):
                        raise
                    refused[n] = str(ex).splitlines()[0][:200]      # torch's backend refuses the shape: recorded, no fallback
                    continue
                e1.synchronize()
                if it >= a.warmup:
                    times[n].append(e0.elapsed_time(e1))
        out = {}
        for n, ts in times.items():
            if n in refused:
                out[n] = dict(refused=refused[n])
                continue
            ms = statistics.median(ts)
            out[n] = dict(ms=round(ms, 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4), tb_per_s=round(acc["bytes"] / (ms * 1e-3) / 1e12, 3))
        cp = out["copy2d"]["ms"]
        for n in ("fwd_epilogue", "fwd_stats", "dgrad", "wgrad"):
            out[n]["over_copy2d"] = round(out[n]["ms"] / cp, 2)
            tn = {"fwd_epilogue": "torch_fwd", "fwd_stats": "torch_fwd", "dgrad": "torch_dgrad", "wgrad": "torch_wgrad"}[n]
            if "ms" in out[tn]:
                out[n]["over_torch"] = round(out[n]["ms"] / out[tn]["ms"], 2)
        row = dict(graph=graph, layer=layer, C=C, hw=hw, k=k, stride=s, **acc, legs=out,
                   copy2d_spread=round((out["copy2d"]["ms_max"] - out["copy2d"]["ms_min"]) / cp, 3))
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()

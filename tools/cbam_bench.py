#!/usr/bin/env python3
"""CBAM micro-benchmark: the forward group (dy_chan_pool_fwd, the fc, dy_spatial_stats_fwd, dy_spatial_gate_fwd) and the backward group
(dy_spatial_gate_bwd_px, dy_spatial_conv_bwd, dy_spatial_gate_bwd_reduce, the fc's backward, dy_spatial_gate_bwd_apply) of ONE CBAM
block (csrc/cbam.hip through nn.modules.CBAM._fwd / _bwd) at B = 32 in bf16, (C, map) = (64, 80^2), (128, 40^2), (256, 20^2), (256, 80^2),
(512, 40^2), (512, 20^2), each beside dy_copy2d moving the budgeted bytes and beside the reference's formula composed from torch
operators on the same channels_last tensors in the same process.  The path is new: ratios are reported, not gated.
  ours    CBAM._fwd with a tape / CBAM._bwd on that tape (the module's own launches, parameter gradients included)
  copy    dy_copy2d with the budget's traffic: 4 map passes forward (pool read, stats read, gate read + write = a plain copy of twice
          the rows), 6 backward (px 2 reads, reduce 2 reads, apply 1 read + 1 write = a plain copy of three times the rows)
  torch   x * sigmoid(fc(avgpool(x))) then u * sigmoid(cv1(cat(mean, max))) under no_grad; its backward through autograd
  pool    the pool alone, dy_chan_pool_fwd (pool_ours) beside dy_gap_fwd (pool_gap, Classify's pool: one thread per channel group and
          image) on the same map: why ChannelAttention has a pool of its own
One process, device events, the legs in rotating order, median of --iters after --warmup, min and max beside the median.

    python tools/cbam_bench.py [--out profiles/cbam_bench.json] [--step NAME=bench_line.json ...]
    python tools/cbam_bench.py --dry-run        # no GPU: shapes and byte accounting only
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = [(64, 80), (128, 40), (256, 20), (256, 80), (512, 40), (512, 20)]


def accounting(B, C, S, es):
    n = B * S * S * C * es                                         # one pass over the map
    return dict(bytes_fwd=4 * n, bytes_bwd=6 * n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the result JSON here (default: print it)")
    ap.add_argument("--step", action="append", default=[], metavar="NAME=FILE", help="merge a bench.py result line as a whole-step figure")
    ap.add_argument("--dry-run", action="store_true", help="no GPU: shapes and accounting; every time is 'not measured'")
    a = ap.parse_args()
    res = dict(batch=a.batch, iters=a.iters, warmup=a.warmup, dtype="bf16", rows=[], step={})
    for name_file in a.step:
        name, path = name_file.split("=", 1)
        lines = []
        if os.path.exists(path):
            with open(path) as f:
                lines = [ln for ln in f.read().splitlines() if ln.startswith("{")]
        res["step"][name] = json.loads(lines[-1]) if lines else "not measured"
    if a.dry_run:
        for C, S in ROWS:
            res["rows"].append(dict(kernel="cbam", C=C, map=S, **accounting(a.batch, C, S, 2), legs="not measured"))
        print(json.dumps(res, indent=1))
        return

    import torch
    import torch.nn.functional as F
    import dedark_yolo_amd as dy
    from dedark_yolo_amd import _C, ops
    from dedark_yolo_amd.nn.modules import CBAM, Tape
    dt = torch.bfloat16
    dy.set_compute_dtype(dt)
    B = a.batch
    res["device"] = torch.cuda.get_device_name(0)
    for C, S in ROWS:
        did, st = ops.dt_id(dt), ops.stream()
        px = B * S * S
        acc = accounting(B, C, S, 2)
        torch.manual_seed(C + S)
        m = CBAM(C, 7).cuda()
        x = ops.as_nhwc(torch.randn(B, C, S, S, device="cuda"), dt)
        gy = ops.as_nhwc(torch.randn(B, C, S, S, device="cuda"), dt)
        big_src, big_dst = torch.empty((4 * px, C), device="cuda", dtype=dt), torch.empty((4 * px, C), device="cuda", dtype=dt)
        p = lambda t: t.data_ptr()
        copy = lambda n: _C.call("dy_copy2d", p(big_src), C, p(big_dst), C, n, C, 0, did, st)
        state = {}

        def ours_fwd():
            state["tape"] = Tape()
            m._fwd(state["tape"], x)

        def ours_bwd():
            m._bwd(state["tape"], gy)

        fcw, fcb, cvw = (t.detach().to(dt) for t in (m.channel_attention.fc.weight, m.channel_attention.fc.bias, m.spatial_attention.cv1.weight))
        leaves = [t.requires_grad_(True) for t in (x.detach().clone(memory_format=torch.channels_last), fcw, fcb, cvw)]

        def fn():
            xx, w1, b1, w2 = leaves
            u = xx * torch.sigmoid(F.conv2d(F.adaptive_avg_pool2d(xx, 1), w1, b1))
            return u * torch.sigmoid(F.conv2d(torch.cat([u.mean(1, keepdim=True), u.max(1, keepdim=True)[0]], 1), w2, padding=3))

        def torch_fwd():
            with torch.no_grad():
                fn()

        def torch_prep():
            state["y"] = fn()

        def torch_bwd():
            torch.autograd.grad(state["y"], leaves, gy)

        legs = {"ours_fwd": (None, ours_fwd), "copy_fwd": (None, lambda: copy(2 * px)), "torch_fwd": (None, torch_fwd),
                "pool_ours": (None, lambda: ops.chan_pool_fwd(x)), "pool_gap": (None, lambda: ops.gap_fwd(x)),
                "ours_bwd": (ours_fwd, ours_bwd), "copy_bwd": (None, lambda: copy(3 * px)), "torch_bwd": (torch_prep, torch_bwd)}
        names = list(legs)
        times = {n: [] for n in names}
        for it in range(a.warmup + a.iters):
            order = names[it % len(names):] + names[:it % len(names)]          # rotating order
            for n in order:
                before, leg = legs[n]
                if before is not None:
                    before()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                leg()
                e1.record()
                e1.synchronize()
                if it >= a.warmup:
                    times[n].append(e0.elapsed_time(e1))
        out = {n: dict(ms=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4)) for n, ts in times.items()}
        verdict = {}
        for d in ("fwd", "bwd"):
            c = out["ours_" + d]
            c["gb_per_s"] = round(acc["bytes_" + d] / (c["ms"] * 1e-3) / 1e9, 1)
            verdict[d] = dict(ours_over_copy=round(c["ms"] / out["copy_" + d]["ms"], 3), ours_over_torch=round(c["ms"] / out["torch_" + d]["ms"], 3))
        verdict["pool"] = dict(ours_over_gap=round(out["pool_ours"]["ms"] / out["pool_gap"]["ms"], 3))
        row = dict(kernel="cbam", C=C, map=S, **acc, legs=out, verdict=verdict)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()

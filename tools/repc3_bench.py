#!/usr/bin/env python3
"""RepConv stage micro-benchmark: dy_bn2_act_fwd / dy_bn2_act_bwd (csrc/bn2act.hip) at the RepC3 shapes of a 640^2 input -- B = 32,
C / map = 128 / 40^2, 64 / 80^2, 256 / 20^2 (the n scale's rows 12 and 18, 15, 21) and 512 / 40^2 (scale l), in bf16 and fp32 -- each
beside dy_copy2d moving the same number of bytes and beside the torch composition on the same tensors in the same process.  The path
is new: there is no earlier kernel of ours, the ratios are reported, not gated.
  ours    the C-ABI entry on dense [B H W, C] matrices; the statistics are those of the tensors (computed once, outside the legs)
  copy    dy_copy2d with the kernel's traffic: 3 tensors (accumulate) for the forward, 8 (a plain copy of four times the rows) for
          the backward's 3 reads + 3 reads + 2 writes -- the HBM-bound floor of this library
  torch   F.silu(F.batch_norm(u) + F.batch_norm(v)) in training mode on channels_last tensors under no_grad; its backward through
          autograd with the same upstream gradient
One process, device events, the legs in rotating order, median of --iters after --warmup, min and max beside the median.

    python tools/repc3_bench.py [--out profiles/repc3_bench.json] [--step NAME=bench_line.json ...]
    python tools/repc3_bench.py --dry-run        # no GPU: shapes and byte accounting only
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = [(dtn, C, S) for dtn in ("bf16", "fp32") for C, S in ((128, 40), (64, 80), (256, 20), (512, 40))]
EPS = 1e-3


def accounting(B, C, S, es):
    n = B * S * S * C * es                                         # one tensor
    return dict(bytes_fwd=3 * n, bytes_bwd=8 * n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the result JSON here (default: print it)")
    ap.add_argument("--step", action="append", default=[], metavar="NAME=FILE", help="merge a bench.py result line as a whole-step figure")
    ap.add_argument("--dry-run", action="store_true", help="no GPU: shapes and accounting; every time is 'not measured'")
    a = ap.parse_args()
    res = dict(batch=a.batch, iters=a.iters, warmup=a.warmup, rows=[], step={})
    for name_file in a.step:
        name, path = name_file.split("=", 1)
        lines = []
        if os.path.exists(path):
            with open(path) as f:
                lines = [ln for ln in f.read().splitlines() if ln.startswith("{")]
        res["step"][name] = json.loads(lines[-1]) if lines else "not measured"
    if a.dry_run:
        for dtn, C, S in ROWS:
            res["rows"].append(dict(kernel="bn2_act", dtype=dtn, C=C, map=S, **accounting(a.batch, C, S, 4 if dtn == "fp32" else 2), legs="not measured"))
        print(json.dumps(res, indent=1))
        return

    import torch
    import torch.nn.functional as F
    from dedark_yolo_amd import _C, ops
    B = a.batch
    res["device"] = torch.cuda.get_device_name(0)
    for dtn, C, S in ROWS:
        dt = dict(fp32=torch.float32, bf16=torch.bfloat16)[dtn]
        did, st = ops.dt_id(dt), ops.stream()
        px = B * S * S
        acc = accounting(B, C, S, 4 if dtn == "fp32" else 2)
        g = torch.Generator(device="cuda").manual_seed(C + S)
        tu, tv, tdy = (torch.randn((px, C), device="cuda", generator=g).to(dt) for _ in range(3))
        y, du, dv = torch.empty_like(tu), torch.empty_like(tu), torch.empty_like(tu)
        big_src, big_dst = torch.empty((4 * px, C), device="cuda", dtype=dt), torch.empty((4 * px, C), device="cuda", dtype=dt)
        aff = []
        for t in (tu, tv):                       # scale, shift, mean, invstd, gamma of a branch
            gamma, beta = torch.rand(C, device="cuda") + 0.5, torch.rand(C, device="cuda") - 0.5
            mean = t.float().mean(0)
            invstd = torch.rsqrt(t.float().var(0, unbiased=False) + EPS)
            aff.append([v.contiguous() for v in (gamma * invstd, beta - mean * gamma * invstd, mean, invstd, gamma)])
        outs = [torch.empty(C, device="cuda") for _ in range(4)]
        ws = torch.empty(ops.bn2_act_bwd_workspace(px, C, dt), device="cuda")
        p = lambda t: t.data_ptr()
        copy = lambda src, dst, n, accum: _C.call("dy_copy2d", p(src), C, p(dst), C, n, C, accum, did, st)
        ours_fwd = lambda: _C.call("dy_bn2_act_fwd", p(tu), C, p(tv), C, p(aff[0][0]), p(aff[0][1]), p(aff[1][0]), p(aff[1][1]), _C.ACT_SILU,
                                   p(y), C, px, C, did, st)
        ours_bwd = lambda: _C.call("dy_bn2_act_bwd", p(tdy), C, p(tu), C, p(tv), C, *(p(t) for t in aff[0]), *(p(t) for t in aff[1]), _C.ACT_SILU,
                                   p(du), C, p(dv), C, *(p(t) for t in outs), p(ws), ws.numel(), px, C, did, st)
        copy_fwd = lambda: copy(tu, y, px, 1)
        copy_bwd = lambda: copy(big_src, big_dst, 4 * px, 0)
        as_map = lambda t: t.view(B, S, S, C).permute(0, 3, 1, 2)
        ru, rv = as_map(tu).detach().requires_grad_(True), as_map(tv).detach().requires_grad_(True)
        par = [t.to(dt).requires_grad_(True) for t in (aff[0][4], aff[0][4] * 0, aff[1][4], aff[1][4] * 0)]
        fn = lambda: F.silu(F.batch_norm(ru, None, None, par[0], par[1], True, 0.0, EPS) + F.batch_norm(rv, None, None, par[2], par[3], True, 0.0, EPS))
        leaves = (ru, rv, *par)
        gy = as_map(tdy)
        state = {}

        def torch_fwd():
            with torch.no_grad():
                fn()

        def torch_prep():
            state["y"] = fn()

        def torch_bwd():
            torch.autograd.grad(state["y"], leaves, gy)

        legs = {"ours_fwd": (None, ours_fwd), "copy_fwd": (None, copy_fwd), "torch_fwd": (None, torch_fwd),
                "ours_bwd": (None, ours_bwd), "copy_bwd": (None, copy_bwd), "torch_bwd": (torch_prep, torch_bwd)}
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
        row = dict(kernel="bn2_act", dtype=dtn, C=C, map=S, **acc, legs=out, verdict=verdict)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()

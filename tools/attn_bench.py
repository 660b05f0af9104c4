#!/usr/bin/env python3
"""Fused attention micro-benchmark: dy_attn_fwd and dy_attn_bwd (csrc/attn.hip) at the C3TR shapes of a 640^2 input -- B = 32,
L = 400 tokens (the P5 map), H = 4 heads of D = 32 / 64 / 72 / 80 (scales n / s, l / m / x), bf16, plus one fp32 row -- beside torch's
scaled_dot_product_attention forward and backward on the same tensors in the same process.  There is no earlier kernel of ours to
compare with: torch's kernel is the yardstick and the ratio is reported, not gated.
  ours    Q | K | V as the three channel slices of one [B, L, 3C] buffer, O and dQ | dK | dV into slices (the layout the model runs)
  torch   F.scaled_dot_product_attention on [B, H, L, D] views of the same buffer; its backward through autograd with the same dO
One process, device events, the legs in rotating order, median of --iters after --warmup, min and max beside the median.  `slower`
says whether ours is slower than torch's by more than the larger max - min spread of the two legs.

    python tools/attn_bench.py [--out profiles/attn_bench.json] [--step NAME=bench_line.json ...]
    python tools/attn_bench.py --dry-run        # no GPU: shapes and flop accounting only
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, H = 400, 4
ROWS = [("bf16", 32), ("bf16", 64), ("bf16", 72), ("bf16", 80), ("fp32", 64)]


def accounting(B, D, es):
    mm = 2.0 * B * H * L * L * D                                   # one L x L x D product
    C = H * D
    return dict(flops_fwd=2 * mm, flops_bwd=7 * mm, bytes_fwd=4 * B * L * C * es, bytes_bwd=8 * B * L * C * es)   # bwd: S and dP in both kernels + dV, dK, dQ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the result JSON here (default: print it)")
    ap.add_argument("--step", action="append", default=[], metavar="NAME=FILE", help="merge a bench.py result line as a whole-step figure")
    ap.add_argument("--dry-run", action="store_true", help="no GPU: shapes and accounting; every time is 'not measured'")
    a = ap.parse_args()
    res = dict(batch=a.batch, L=L, H=H, iters=a.iters, warmup=a.warmup, rows=[], step={})
    for name_file in a.step:
        name, path = name_file.split("=", 1)
        lines = []
        if os.path.exists(path):
            with open(path) as f:
                lines = [ln for ln in f.read().splitlines() if ln.startswith("{")]
        res["step"][name] = json.loads(lines[-1]) if lines else "not measured"
    if a.dry_run:
        for dtn, D in ROWS:
            res["rows"].append(dict(dtype=dtn, D=D, **accounting(a.batch, D, 4 if dtn == "fp32" else 2), legs="not measured"))
        print(json.dumps(res, indent=1))
        return

    import torch
    import torch.nn.functional as F
    from dedark_yolo_amd import _C, ops
    B = a.batch
    res["device"] = torch.cuda.get_device_name(0)
    for dtn, D in ROWS:
        dt = dict(fp32=torch.float32, bf16=torch.bfloat16)[dtn]
        did, C, scale = ops.dt_id(dt), H * D, D ** -0.5
        acc = accounting(B, D, 4 if dtn == "fp32" else 2)
        g = torch.Generator(device="cuda").manual_seed(D)
        qkv = torch.randn((B, L, 3 * C), device="cuda", generator=g).to(dt)
        dout = torch.randn((B, L, C), device="cuda", generator=g).to(dt)
        o = torch.empty((B, L, C), device="cuda", dtype=dt)
        gbuf = torch.empty((B, L, 3 * C), device="cuda", dtype=dt)
        lse = torch.empty(B * H * L, device="cuda", dtype=torch.float32)
        es = qkv.element_size()
        p = [qkv.data_ptr() + i * C * es for i in range(3)]
        gp = [gbuf.data_ptr() + i * C * es for i in range(3)]
        st = ops.stream()

        def ours_fwd():
            _C.call("dy_attn_fwd", p[0], 3 * C, p[1], 3 * C, p[2], 3 * C, o.data_ptr(), C, lse.data_ptr(), B, L, H, D, scale, did, st)

        def ours_bwd():
            _C.call("dy_attn_bwd", p[0], 3 * C, p[1], 3 * C, p[2], 3 * C, o.data_ptr(), C, dout.data_ptr(), C, lse.data_ptr(), gp[0], 3 * C, gp[1], 3 * C,
                    gp[2], 3 * C, B, L, H, D, scale, did, st)

        tq, tk, tv = (qkv[..., i * C:(i + 1) * C].reshape(B, L, H, D).transpose(1, 2).detach().requires_grad_(True) for i in range(3))
        tdo = dout.reshape(B, L, H, D).transpose(1, 2)
        state = {}

        def torch_fwd():
            with torch.no_grad():
                F.scaled_dot_product_attention(tq, tk, tv)

        def torch_prep():
            state["y"] = F.scaled_dot_product_attention(tq, tk, tv)

        def torch_bwd():
            torch.autograd.grad(state["y"], (tq, tk, tv), tdo)

        ours_fwd()                                               # O and LSE the backward reads
        legs = {"ours_fwd": (None, ours_fwd), "torch_fwd": (None, torch_fwd), "ours_bwd": (None, ours_bwd), "torch_bwd": (torch_prep, torch_bwd)}
        names = list(legs)
        times = {n: [] for n in names}
        for it in range(a.warmup + a.iters):
            order = names[it % len(names):] + names[:it % len(names)]          # rotating order
            for n in order:
                before, fn = legs[n]
                if before is not None:
                    before()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if it >= a.warmup:
                    times[n].append(e0.elapsed_time(e1))
        out = {n: dict(ms=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4)) for n, ts in times.items()}
        for d in ("fwd", "bwd"):
            out["ours_" + d]["tflops"] = round(acc["flops_" + d] / (out["ours_" + d]["ms"] * 1e-3) / 1e12, 2)
        verdict = {}
        for d in ("fwd", "bwd"):
            c, t = out["ours_" + d], out["torch_" + d]
            spread = max(c["ms_max"] - c["ms_min"], t["ms_max"] - t["ms_min"])
            verdict[d] = dict(ours_over_torch=round(c["ms"] / t["ms"], 3), spread_ms=round(spread, 4), slower=bool(c["ms"] > t["ms"] + spread))
        row = dict(dtype=dtn, D=D, **acc, legs=out, verdict=verdict)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()

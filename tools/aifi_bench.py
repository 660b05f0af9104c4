#!/usr/bin/env python3
"""Transformer-encoder-layer micro-benchmark: dy_add_layernorm_fwd / _bwd and dy_gelu_fwd / _bwd (csrc/layernorm.hip) at the AIFI
shapes of a 640^2 input -- B = 32, L = 400 tokens (the P5 map), C = 256 / 512 / 640 (scales n / s, l / x) for LayerNorm and the
feed-forward width cm = 1024 for GELU, in bf16 and fp32 -- each beside dy_copy2d moving the same number of bytes and beside torch's
own kernels on the same tensors in the same process.  The path is new: there is no earlier kernel of ours, the ratios are reported,
not gated.
  ours    the C-ABI entry on dense [B L, C] matrices
  copy    dy_copy2d with the kernel's traffic: 3 tensors (accumulate) for add+LayerNorm forward and GELU backward, 2 for GELU
          forward, 4 (a plain copy of twice the rows) for add+LayerNorm backward -- the HBM-bound floor of this library
  torch   F.layer_norm(a + b) / F.gelu(u) under no_grad; their backward through autograd with the same upstream gradient
One process, device events, the legs in rotating order, median of --iters after --warmup, min and max beside the median.

    python tools/aifi_bench.py [--out profiles/aifi_bench.json] [--step NAME=bench_line.json ...]
    python tools/aifi_bench.py --dry-run        # no GPU: shapes and byte accounting only
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L = 400
ROWS = [(k, dtn, C) for dtn in ("bf16", "fp32") for k, C in (("ln", 256), ("ln", 512), ("ln", 640), ("gelu", 1024))]


def accounting(kind, B, C, es):
    n = B * L * C * es                                             # one tensor
    return dict(bytes_fwd=(3 if kind == "ln" else 2) * n, bytes_bwd=(4 if kind == "ln" else 3) * n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the result JSON here (default: print it)")
    ap.add_argument("--step", action="append", default=[], metavar="NAME=FILE", help="merge a bench.py result line as a whole-step figure")
    ap.add_argument("--dry-run", action="store_true", help="no GPU: shapes and accounting; every time is 'not measured'")
    a = ap.parse_args()
    res = dict(batch=a.batch, L=L, iters=a.iters, warmup=a.warmup, rows=[], step={})
    for name_file in a.step:
        name, path = name_file.split("=", 1)
        lines = []
        if os.path.exists(path):
            with open(path) as f:
                lines = [ln for ln in f.read().splitlines() if ln.startswith("{")]
        res["step"][name] = json.loads(lines[-1]) if lines else "not measured"
    if a.dry_run:
        for kind, dtn, C in ROWS:
            res["rows"].append(dict(kernel=kind, dtype=dtn, C=C, **accounting(kind, a.batch, C, 4 if dtn == "fp32" else 2), legs="not measured"))
        print(json.dumps(res, indent=1))
        return

    import torch
    import torch.nn.functional as F
    from dedark_yolo_amd import _C, ops
    B = a.batch
    rows = B * L
    res["device"] = torch.cuda.get_device_name(0)
    for kind, dtn, C in ROWS:
        dt = dict(fp32=torch.float32, bf16=torch.bfloat16)[dtn]
        did, st = ops.dt_id(dt), ops.stream()
        acc = accounting(kind, B, C, 4 if dtn == "fp32" else 2)
        g = torch.Generator(device="cuda").manual_seed(C)
        ta, tb, tdy = (torch.randn((rows, C), device="cuda", generator=g).to(dt) for _ in range(3))
        y, dz = torch.empty_like(ta), torch.empty_like(ta)
        big_src, big_dst = torch.empty((2 * rows, C), device="cuda", dtype=dt), torch.empty((2 * rows, C), device="cuda", dtype=dt)
        gamma, beta = torch.rand(C, device="cuda") + 0.5, torch.rand(C, device="cuda")
        stats = torch.empty(2 * rows, device="cuda", dtype=torch.float32)
        dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        parts = ops.ln_parts(rows, C)
        scratch = torch.empty(parts * 2 * C, device="cuda")
        p = lambda t: t.data_ptr()
        copy = lambda src, dst, n, accum: _C.call("dy_copy2d", p(src), C, p(dst), C, n, C, accum, did, st)
        state = {}
        if kind == "ln":
            ours_fwd = lambda: _C.call("dy_add_layernorm_fwd", p(ta), C, p(tb), C, p(gamma), p(beta), p(y), C, p(stats), rows, C, 1e-5, did, st)
            ours_bwd = lambda: _C.call("dy_add_layernorm_bwd", p(ta), C, p(tb), C, p(stats), p(gamma), p(tdy), C, p(dz), C, 0, p(dg), p(db),
                                       p(scratch), scratch.numel(), rows, C, did, st)
            copy_fwd = lambda: copy(ta, y, rows, 1)
            copy_bwd = lambda: copy(big_src, big_dst, 2 * rows, 0)
            ra, rb = ta.detach().requires_grad_(True), tb.detach().requires_grad_(True)
            gm, bt = gamma.to(dt).requires_grad_(True), beta.to(dt).requires_grad_(True)
            fn = lambda: F.layer_norm(ra + rb, (C,), gm, bt, 1e-5)
            leaves = (ra, rb, gm, bt)
        else:
            ours_fwd = lambda: _C.call("dy_gelu_fwd", p(ta), C, p(y), C, rows, C, did, st)
            ours_bwd = lambda: _C.call("dy_gelu_bwd", p(ta), C, p(tdy), C, p(dz), C, rows, C, did, st)
            copy_fwd = lambda: copy(ta, y, rows, 0)
            copy_bwd = lambda: copy(ta, dz, rows, 1)
            ra = ta.detach().requires_grad_(True)
            fn = lambda: F.gelu(ra)
            leaves = (ra,)

        def torch_fwd():
            with torch.no_grad():
                fn()

        def torch_prep():
            state["y"] = fn()

        def torch_bwd():
            torch.autograd.grad(state["y"], leaves, tdy)

        ours_fwd()                                               # the statistics the backward reads
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
        row = dict(kernel=kind, dtype=dtn, C=C, **acc, legs=out, verdict=verdict)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()

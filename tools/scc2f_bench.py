#!/usr/bin/env python3
"""CRU convolution group micro-benchmark: the five convolutions of SCConv's channel reconstruction unit (squeeze1, squeeze2,
GWC + PWC1, PWC2) at the SCConv widths of yolov8l-SCC2f -- C = 64 / 128 / 256 on 160^2 / 80^2 / 40^2 maps, B = 32, bf16 -- on two
legs that both builds contain:
  cru       the dy_cru_conv_* kernels (ops.cru_conv_forward / cru_conv_backward): GWC + PWC1 in one accumulator
  composed  the generic conv routes on channel slices, as MFRU runs them (SCConv._composed_cru_fwd / _composed_cru_bwd): two 3x3
            calls on C/8-channel slices, a PWC1 call and a dy_copy2d(accumulate)
Timed per leg: the group's forward, and its backward (data and weight gradients of all five convolutions, which the composed leg's
conv_backward computes in one call each and cannot give separately); for the cru leg also the data gradients and the weight
gradients alone (C-ABI calls).  The SRU, the moments and the CRU tail are the same kernels on both legs and are not timed.
One process, device events, the legs in rotating order, median of --iters after --warmup, min and max beside the median.  A leg is
FASTER only if its median is lower by more than the larger max - min spread of the two legs; `verdict` says which, per width and
direction, and `family` is the rule for SCConv._cru at widths that are multiples of 64 (switch only if cru is faster in both).

    python tools/scc2f_bench.py [--out profiles/scc2f_bench.json] [--step NAME=bench_line.json ...]
    python tools/scc2f_bench.py --dry-run        # no GPU: shapes and flop accounting only
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(64, 160), (128, 80), (256, 40)]          # (SCConv width, H = W): model.2 / model.4 / model.6 of yolov8l-SCC2f at 640


def accounting(B, C, hw, es):
    px = B * hw * hw
    h, q, e = C // 2, C // 4, C // 8
    macs = px * (2 * h * q + C * (9 * e + q) + 3 * q * q)            # squeeze1 + squeeze2, GWC + PWC1, PWC2
    return dict(pixels=px, flops_fwd=2 * macs, bytes_fwd=px * (C + q + 2 * C) * es,      # reads y, writes up' and the 2C buffer
                K_up=9 * e + q)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the result JSON here (default: print it)")
    ap.add_argument("--step", action="append", default=[], metavar="NAME=FILE", help="merge a bench.py result line as a whole-step figure")
    ap.add_argument("--dry-run", action="store_true", help="no GPU: shapes and accounting; every time is 'not measured'")
    a = ap.parse_args()
    es = 4 if a.dtype == "fp32" else 2
    res = dict(dtype=a.dtype, batch=a.batch, iters=a.iters, warmup=a.warmup, shapes=[], step={})
    for name_file in a.step:
        name, path = name_file.split("=", 1)
        lines = []
        if os.path.exists(path):
            with open(path) as f:
                lines = [ln for ln in f.read().splitlines() if ln.startswith("{")]
        res["step"][name] = json.loads(lines[-1]) if lines else "not measured"
    if a.dry_run:
        for C, hw in SHAPES:
            res["shapes"].append(dict(C=C, hw=hw, **accounting(a.batch, C, hw, es), legs="not measured"))
        print(json.dumps(res, indent=1))
        return

    import torch
    import dedark_yolo_amd as dy
    from dedark_yolo_amd import _C, ops
    from dedark_yolo_amd.nn.modules import SCConv, Tape
    dt = dict(fp32=torch.float32, bf16=torch.bfloat16, fp16=torch.float16)[a.dtype]
    dy.set_compute_dtype(dt)
    did, B = ops.dt_id(dt), a.batch
    res["device"] = torch.cuda.get_device_name(0)

    for C, hw in SHAPES:
        acc = accounting(B, C, hw, es)
        h, q, e = C // 2, C // 4, C // 8
        torch.manual_seed(C)
        m = SCConv(C).cuda().train()
        cru = m.CRU
        g = torch.Generator(device="cuda").manual_seed(C + hw)
        y = (torch.rand((B, hw, hw, C), device="cuda", generator=g) * 2 - 1).to(dt).permute(0, 3, 1, 2)
        dbuf0 = (torch.rand((B, hw, hw, 2 * C), device="cuda", generator=g) * 2 - 1).to(dt).permute(0, 3, 1, 2)
        buf = ops.empty_nhwc(B, 2 * C, hw, hw, dt, "cuda")
        dyo = ops.empty_nhwc(B, C, hw, hw, dt, "cuda")

        def cru_fwd(tape):
            sq1 = ops.cru_conv_forward(tape, y[:, :h], None, None, cru.squeeze1.weight)
            low = ops.cru_conv_forward(tape, y[:, h:], None, None, cru.squeeze2.weight, out=buf[:, 2 * C - q:])
            ops.cru_conv_forward(tape, sq1, cru.GWC.weight, cru.GWC.bias, cru.PWC1.weight, G=2, out=buf[:, :C])
            ops.cru_conv_forward(tape, low, None, None, cru.PWC2.weight, out=buf[:, C:2 * C - q])

        def cru_bwd(tape, dbuf):
            ops.cru_conv_backward(tape, dbuf[:, C:2 * C - q], dx_out=dbuf[:, 2 * C - q:], accumulate=True)
            dsq1 = ops.cru_conv_backward(tape, dbuf[:, :C])
            ops.cru_conv_backward(tape, dbuf[:, 2 * C - q:], dx_out=dyo[:, h:])
            ops.cru_conv_backward(tape, dsq1, dx_out=dyo[:, :h])

        state = {}

        def prep(leg):                                  # an untimed forward that leaves the tape the backward consumes
            tape = Tape()
            state["views"] = cru_fwd(tape) if leg == "cru" else m._composed_cru_fwd(tape, y, buf)
            state["tape"], state["dbuf"] = tape, dbuf0.clone()

        # the cru leg's gradients alone, through the C-ABI
        st = ops.stream()
        sq1 = ops.cru_conv_forward(None, y[:, :h], None, None, cru.squeeze1.weight)
        dsq1 = ops.empty_nhwc(B, q, hw, hw, dt, "cuda")
        scratch = ops.wgrad_scratch(torch.device("cuda", 0), tag=st)
        convs = [(y[:, :h], dsq1, dyo[:, :h], None, None, cru.squeeze1.weight, 1), (y[:, h:], dbuf0[:, 2 * C - q:], dyo[:, h:], None, None, cru.squeeze2.weight, 1),
                 (sq1, dbuf0[:, :C], dsq1, cru.GWC.weight, cru.GWC.bias, cru.PWC1.weight, 2),
                 (dbuf0[:, 2 * C - q:], dbuf0[:, C:2 * C - q], ops.empty_nhwc(B, q, hw, hw, dt, "cuda"), None, None, cru.PWC2.weight, 1)]
        gw = [(None if w3 is None else torch.empty_like(w3), None if b is None else torch.empty_like(b), torch.empty_like(w1))
              for _, _, _, w3, b, w1, _ in convs]

        def dims(x, w3, w1, G):
            return G, w1.shape[0] // G, (0 if w3 is None else w3.shape[1]), w1.shape[1]

        def cru_dgrad_only():
            for x, d, dx, w3, b, w1, G in convs:
                wp = ops._cru_packed(w3, w1, G, True, dt)
                _C.call("dy_cru_conv_dgrad", d.data_ptr(), ops.ld_of(d), wp.data_ptr(), dx.data_ptr(), ops.ld_of(dx), B, hw, hw, *dims(x, w3, w1, G), 0, did, st)

        def cru_wgrad_only():
            for (x, d, dx, w3, b, w1, G), (g3, gb, g1) in zip(convs, gw):
                _C.call("dy_cru_conv_wgrad", x.data_ptr(), ops.ld_of(x), d.data_ptr(), ops.ld_of(d), ops.ptr(g3), ops.ptr(gb), g1.data_ptr(), B, hw, hw,
                        *dims(x, w3, w1, G), scratch.data_ptr(), scratch.numel(), did, st)

        legs = {
            "cru_fwd": (None, lambda: cru_fwd(None)),
            "composed_fwd": (None, lambda: m._composed_cru_fwd(None, y, buf)),
            "cru_bwd": (lambda: prep("cru"), lambda: cru_bwd(state["tape"], state["dbuf"])),
            "composed_bwd": (lambda: prep("composed"), lambda: m._composed_cru_bwd(state["tape"], state["dbuf"], dyo, *state["views"])),
            "cru_dgrad": (None, cru_dgrad_only),
            "cru_wgrad": (None, cru_wgrad_only),
        }
        names = list(legs)
        times = {n: [] for n in names}
        with torch.no_grad():
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
        out = {}
        for n, ts in times.items():
            ms = statistics.median(ts)
            out[n] = dict(ms=round(ms, 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
        out["cru_fwd"]["tflops"] = round(acc["flops_fwd"] / (out["cru_fwd"]["ms"] * 1e-3) / 1e12, 2)
        out["composed_fwd"]["tflops"] = round(acc["flops_fwd"] / (out["composed_fwd"]["ms"] * 1e-3) / 1e12, 2)
        verdict = {}
        for d in ("fwd", "bwd"):
            c, o = out["cru_" + d], out["composed_" + d]
            spread = max(c["ms_max"] - c["ms_min"], o["ms_max"] - o["ms_min"])
            verdict[d] = dict(cru_over_composed=round(c["ms"] / o["ms"], 3), spread_ms=round(spread, 4),
                              faster="cru" if c["ms"] < o["ms"] - spread else "composed" if o["ms"] < c["ms"] - spread else "neither (inside the spread)")
        row = dict(C=C, hw=hw, **acc, legs=out, verdict=verdict)
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
    both = all(r["verdict"][d]["faster"] == "cru" for r in res["shapes"] for d in ("fwd", "bwd"))
    res["family"] = ("switch the C % 64 == 0 widths of the C2f family to the cru kernels" if both else
                     "the C % 64 == 0 widths keep the composed path: the cru kernels are not faster by more than the spread at every width and direction")
    print(res["family"])
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()

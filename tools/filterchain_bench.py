#!/usr/bin/env python3
"""Front-end filter-chain micro-benchmark: the general pointwise kernels of csrc/filterchain.hip (dy_filter_chain_fwd/bwd) beside the
fused pair of the default chain (dy_filters_pointwise_fwd/bwd, csrc/frontend.hip), at B = 64, 640 x 640, f32 images, A / IcA null.
Legs:
  fused_fwd / fused_bwd            today's pair on the default chain [DF, W, G, Ct]
  chain_fwd / chain_bwd            the general entry on the same chain
  chain_tone_fwd / chain_tone_bwd  the general entry with T added: [DF, W, G, T, Ct]
  copy2d                           dy_copy2d moving the forward's bytes (one image read, one written): the project's own
                                   achieved-bandwidth yardstick; its spread over the run is the noise floor for any claim
One process, device events, legs in rotating order (the first leg of an iteration moves on by one each time), median of --iters
after --warmup, [min .. max] beside each median.  Bytes from the shapes: a forward reads and writes one [B,3,H,W] f32 image, a
backward reads two (x and the upstream gradient) and writes one; parameters are noise.  Nothing is gated on these numbers: the
default chain keeps the fused pair whatever the general kernel costs.

    python tools/filterchain_bench.py [--out profiles/filterchain_bench.json] [--step NAME=bench_line.json ...]
    python tools/filterchain_bench.py --dry-run        # no GPU: shapes and byte accounting only
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CODES = dict(DF=1, W=2, G=3, T=4, Ct=5)
DEFAULT_PW, TONE_PW = ("DF", "W", "G", "Ct"), ("DF", "W", "G", "T", "Ct")


def word(names):
    return sum(CODES[n] << (4 * k) for k, n in enumerate(names))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fast-math", type=int, default=1, choices=[0, 1], help="1: the hardware log2 / exp2 / rcp of the 16-bit training modes")
    ap.add_argument("--out", default=None, help="write the result JSON here (default: print it)")
    ap.add_argument("--step", action="append", default=[], metavar="NAME=FILE", help="merge a bench.py result line as a whole-step figure")
    ap.add_argument("--dry-run", action="store_true", help="no GPU: shapes and byte accounting; every time is 'not measured'")
    a = ap.parse_args()
    B, S = a.batch, a.imgsz
    img_bytes = B * 3 * S * S * 4
    nbytes = dict(fused_fwd=2 * img_bytes, chain_fwd=2 * img_bytes, chain_tone_fwd=2 * img_bytes, copy2d=2 * img_bytes,
                  fused_bwd=3 * img_bytes, chain_bwd=3 * img_bytes, chain_tone_bwd=3 * img_bytes)
    res = dict(batch=B, imgsz=S, iters=a.iters, warmup=a.warmup, fast_math=a.fast_math, bytes=nbytes, step={})
    for name_file in a.step:
        name, path = name_file.split("=", 1)
        with open(path) as f:
            lines = [ln for ln in f.read().splitlines() if ln.startswith("{")]
        res["step"][name] = json.loads(lines[-1]) if lines else "not measured"
    if a.dry_run:
        res["legs"] = "not measured"
        print(json.dumps(res, indent=1))
        return

    import torch
    from dedark_yolo_amd import _C, ops
    res["device"] = torch.cuda.get_device_name(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand((B, 3, S, S), device="cuda", generator=g) * 1.3 - 0.2
    gy = torch.rand((B, 3, S, S), device="cuda", generator=g) * 2 - 1
    y, dx = torch.empty_like(x), torch.empty_like(x)
    feat = (torch.rand((B, 16), device="cuda", generator=g) * 3 - 1.5).contiguous()
    params, tone = torch.empty((B, 8), device="cuda"), torch.empty((B, 8), device="cuda")
    dp, dtn = torch.zeros((B, 8), dtype=torch.float64, device="cuda"), torch.zeros((B, 8), dtype=torch.float64, device="cuda")
    st, fm = ops.stream(), a.fast_math
    _C.call("dy_filter_params_fwd", feat.data_ptr(), 16, params.data_ptr(), B, st)
    _C.call("dy_tone_params_fwd", feat.data_ptr(), 16, tone.data_ptr(), B, st)
    n_copy = B * 3 * S * S // 8
    P = lambda t: t.data_ptr()
    wd, wt = word(DEFAULT_PW), word(TONE_PW)
    legs = {
        "fused_fwd": lambda: _C.call("dy_filters_pointwise_fwd", P(x), P(params), None, None, P(y), B, S, S, fm, st),
        "fused_bwd": lambda: _C.call("dy_filters_pointwise_bwd", P(x), P(params), None, None, P(gy), P(dx), P(dp), B, S, S, 0, fm, st),
        "chain_fwd": lambda: _C.call("dy_filter_chain_fwd", P(x), P(params), None, None, None, wd, P(y), B, S, S, fm, st),
        "chain_bwd": lambda: _C.call("dy_filter_chain_bwd", P(x), P(params), None, None, None, wd, P(gy), None, 0, 0, P(dx), P(dp), None, B, S,
                                     S, 0, fm, st),
        "chain_tone_fwd": lambda: _C.call("dy_filter_chain_fwd", P(x), P(params), P(tone), None, None, wt, P(y), B, S, S, fm, st),
        "chain_tone_bwd": lambda: _C.call("dy_filter_chain_bwd", P(x), P(params), P(tone), None, None, wt, P(gy), None, 0, 0, P(dx), P(dp),
                                          P(dtn), B, S, S, 0, fm, st),
        "copy2d": lambda: _C.call("dy_copy2d", P(x), 8, P(y), 8, n_copy, 8, 0, _C.DY_F32, st),
    }
    names = list(legs)
    times = {n: [] for n in names}
    for it in range(a.warmup + a.iters):
        for k in range(len(names)):
            n = names[(it + k) % len(names)]                      # rotating order
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            legs[n]()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[n].append(e0.elapsed_time(e1))
    out = {}
    for n, ts in times.items():
        ms = statistics.median(ts)
        out[n] = dict(ms=round(ms, 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4), tb_per_s=round(nbytes[n] / (ms * 1e-3) / 1e12, 3))
    cp = out["copy2d"]
    res["copy2d_spread"] = round((cp["ms_max"] - cp["ms_min"]) / cp["ms"], 3)
    for d in ("fwd", "bwd"):
        out["chain_" + d]["over_fused"] = round(out["chain_" + d]["ms"] / out["fused_" + d]["ms"], 3)
        out["chain_tone_" + d]["over_fused"] = round(out["chain_tone_" + d]["ms"] / out["fused_" + d]["ms"], 3)
    res["legs"] = out
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()

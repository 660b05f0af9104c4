"""Cost of the fused optimizer steps on a flat state of the yolov8l size.  One JSON line.

  python tools/optim_bench.py [--model yolov8l.yaml] [--steps 20] [--warmup 3] [--out profiles/optim_bench.json]

n and the mix of parameter groups come from FlatState(DetectionModel(model)); the values are synthetic.  One process, device events
around each call, the legs interleaved (every round runs each leg once, in rotating order, so drift and a neighbour's dirty lines
hit all of them alike), median of `--steps` rounds after `--warmup`: dy_sgd_step_scaled, dy_adamw_step_scaled and dy_optim_step with
each of its five rules (its one-thread scalar launch included), every leg on buffers of its own with clipping and the EMA on.  Per
leg: ms (median, min, max), the bytes per element its rule reads and writes, and the achieved TB/s.  The yardstick of the five rules
is the adamw leg of the same run: they move the same 37 bytes per element (p, g, two buffers and the EMA read, the group id, all but
g written back), so they should take the same time within the run's own spread (`spread_ms`: the largest max - min of any leg).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# bytes per element: f32 reads of p, g, the state buffers and the EMA + one group id byte, f32 writes of all of them but g
BYTES = dict(sgd=4 * 4 + 1 + 3 * 4, adamw=5 * 4 + 1 + 4 * 4)
RULES = ("Adam", "Adamax", "NAdam", "RAdam", "RMSProp")


def run(model, steps, warmup):
    import torch
    from dedark_yolo_amd._C import OPT_RULES, call
    from dedark_yolo_amd.engine.trainer import FlatState
    from dedark_yolo_amd.nn import tasks
    from dedark_yolo_amd.ops import ptr, stream
    flat = FlatState(tasks.DetectionModel(tasks.yaml_model_load(model), nc=80), with_ema=False)          # on the CPU: sizes only
    n, gid = flat.n, flat.gid.cuda()
    mix = [int((flat.gid == k).sum()) for k in range(3)]
    del flat
    gen = torch.Generator(device="cuda").manual_seed(0)
    p0 = torch.randn(n, device="cuda", generator=gen) * 0.05
    g = torch.randn(n, device="cuda", generator=gen) * 1e-2                                             # norm ~66: the clip is active
    ss = torch.zeros(1, dtype=torch.float64, device="cuda")
    call("dy_sumsq", ptr(g), n, ptr(ss), stream())
    lr, wd, d = (1e-3, 1e-3, 1e-3), 5e-4, 0.999

    def leg(name):
        p, m, m2, ema = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), p0.clone()
        if name == "sgd":
            return lambda t: call("dy_sgd_step_scaled", ptr(p), ptr(g), ptr(m), ptr(ema), ptr(gid), *lr, wd, 0.0, 0.0, 0.9, 1, d, ptr(ss),
                                  10.0, 1.0, None, n, stream())
        if name == "adamw":
            return lambda t: call("dy_adamw_step_scaled", ptr(p), ptr(g), ptr(m), ptr(m2), ptr(ema), ptr(gid), *lr, wd, 0.0, 0.0, 0.9, 0.999,
                                  1e-8, t, d, ptr(ss), 10.0, 1.0, None, n, stream())
        st = torch.zeros(8, dtype=torch.float64, device="cuda")
        st[1] = 1.0
        return lambda t: call("dy_optim_step", OPT_RULES[name], ptr(p), ptr(g), ptr(m), ptr(m2), ptr(ema), ptr(gid), *lr, wd, 0.0, 0.0, 0.9,
                              0.99 if name == "RMSProp" else 0.999, 1e-8, 0.004, d, ptr(ss), 10.0, 1.0, None, ptr(st), n, stream())

    legs = {name: leg(name) for name in ("sgd", "adamw") + RULES}
    times = {name: [] for name in legs}
    names = list(legs)
    for t in range(1, warmup + steps + 1):
        for name in names[t % len(names):] + names[:t % len(names)]:       # rotated: no leg always runs behind the same neighbour
            fn = legs[name]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(t)
            e1.record()
            if t > warmup:
                times[name].append((e0, e1))
    torch.cuda.synchronize()
    out = dict(model=model, n=n, group_elements=dict(decayed=mix[0], norm=mix[1], bias=mix[2]), steps=steps, warmup=warmup,
               device=torch.cuda.get_device_name(0), legs={})
    for name, ev in times.items():
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        med, b = ms[len(ms) // 2], BYTES["sgd" if name == "sgd" else "adamw"]
        out["legs"][name] = dict(ms=round(med, 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4), bytes_per_element=b,
                                 tb_per_s=round(n * b / (med * 1e-3) / 1e12, 3))
    ref = out["legs"]["adamw"]["ms"]
    out["spread_ms"] = round(max(v["ms_max"] - v["ms_min"] for v in out["legs"].values()), 4)
    out["over_adamw"] = {name: round(out["legs"][name]["ms"] / ref, 3) for name in RULES}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="yolov8l.yaml")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    a = ap.parse_args()
    line = json.dumps(run(a.model, a.steps, a.warmup))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

"""Records {C-ABI entry: GPU kernel symbol} of every (dtype, shape) the default-dispatch tests of tests/test_gpu_conv_kernels.py run,
as "<dtype>:<shape id>" -> routes, into tests/golden/g22_conv_routes.json (the tests assert equality with it).  Run it against the
library of the commit BEFORE a dispatch change: build that commit's csrc with `make OUT=<dir>/libdedark_yolo.so OBJDIR=<dir>/obj`, then
    DY_LIB_DIR=<dir> python tools/conv_route_snapshot.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_gpu_conv_kernels as t  # noqa: E402

snap = {}
for dtype, shapes in t.ROUTE_CASES:
    for shape in shapes:
        routes = {}
        t._case(dtype, *shape, routes=routes)
        snap[t.route_key(dtype, shape)] = routes
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "g22_conv_routes.json")
with open(out, "w") as f:
    json.dump(snap, f, indent=0, sort_keys=True)
    f.write("\n")
print(len(snap), "cases ->", out)

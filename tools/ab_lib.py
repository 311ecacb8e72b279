"""A/B of two or more builds of the library on config 2 in ONE process, interleaved rounds (cdna guide rule 24).

   python tools/ab_lib.py A.so B.so [spp]                       five rounds, the libraries in the given order in each
   python tools/ab_lib.py A.so B.so [spp] --pairs N --json F    two warm-up rounds, then N pairs (A, B) with the order swapped every pair; the
                                                                pairs, both medians and A's own spread (max - min) go to F.  A = the parent's
                                                                build; `gain` = the median difference exceeds three times that spread
"""
import argparse
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("what", nargs="+", metavar="LIB.so | SPP", help="file names under amber_amd/lib, and optionally the samples per pixel (default 256)")
ap.add_argument("--pairs", type=int, default=0, metavar="N")
ap.add_argument("--json", default=None, metavar="FILE")
args = ap.parse_args()
libs = [w for w in args.what if w.endswith(".so")]
numbers = [w for w in args.what if not w.endswith(".so")]
if len(numbers) > 1 or not all(w.isdigit() for w in numbers) or not libs or (args.pairs and len(libs) != 2):
    ap.error("expected library file names (two with --pairs) and at most one sample count")
spp = int(numbers[0]) if numbers else 256

import amber_amd.api as api

handles = {}
for path in libs:
    api._lib = None
    api._LIB_PATH = api._ROOT / "lib" / path
    import amber_amd as A
    lib = A.load_library()
    sc = A.HostScene.cornell_box()
    handles[path] = (lib, sc, A.PathTracer(sc, A.Sensor.default(1024, 1024)))


def kernel_ms(path):
    lib, sc, pt = handles[path]
    api._lib = lib
    pt.clear()
    pt.render_pass(0, spp)
    pt.sync()
    return pt.kernel_time()[1]


res = {path: [] for path in libs}
if args.pairs:
    a, b = libs
    for rnd in range(2):
        for path in (a, b):
            kernel_ms(path)
    pairs = []
    for k in range(args.pairs):
        t = {}
        for path in ((a, b) if k % 2 == 0 else (b, a)):
            t[path] = kernel_ms(path)
        pairs.append([t[a], t[b]])
        res[a].append(t[a])
        res[b].append(t[b])
    out = {"parent": a, "new": b, "spp": spp, "pairs": pairs, "parent_median": statistics.median(res[a]), "new_median": statistics.median(res[b]),
           "parent_min": min(res[a]), "parent_max": max(res[a]), "new_min": min(res[b]), "new_max": max(res[b])}
    out["parent_spread"] = out["parent_max"] - out["parent_min"]
    out["gain"] = bool(out["parent_median"] - out["new_median"] > 3.0 * out["parent_spread"])
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(out) + "\n")
else:
    for rnd in range(5):
        for path in libs:
            res[path].append(kernel_ms(path))
for path in libs:
    print("%-28s median %.2f ms  min %.2f  (%s)" % (path, statistics.median(res[path]), min(res[path]), " ".join("%.1f" % x for x in res[path])))
sys.stdout.flush()
os._exit(0)   # several copies of the library are loaded: skip their exit-time teardown (it can abort)

#!/usr/bin/env python3
"""Host build against device build (AMBER_PT_FLAG_DEVICE_BUILD) of engine BVH's tree: create time, tree stage, tree size, render kernel time.

For config 3's scene (1M spheres), the terrain and the room mesh: median of 5 creates with and without the flag after one warm-up create
(code objects loaded), n_nodes / depth of either tree, the render kernel time of either tree at the bench's frame and --spp, and the sample
count at which host build + render overtakes device build + render.  Writes the table to stdout (profiles/device_build.txt keeps one run).

    AMBER_AMD_LIB=libamber_hip.so python tools/device_build.py [--spp 64] [--scenes spheres,terrain,room]
"""
import argparse
import statistics
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import amber_amd as A                                    # noqa: E402
from amber_amd import scenes, workloads                  # noqa: E402


def measure(hs, W, H, seed, spp, device):
    flags = A.PT_FLAG_DEVICE_BUILD if device else 0
    A.PathTracer(hs, A.Sensor.default(W, H), seed=seed, flags=flags).close()
    create, tree = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        pt = A.PathTracer(hs, A.Sensor.default(W, H), seed=seed, flags=flags)
        create.append((time.perf_counter() - t0) * 1e3)
        info = pt.build_info()
        tree.append(info["tree_ms"])
        if len(create) < 5:
            pt.close()
    pt.render_pass(0, spp)
    pt.sync()
    pt.clear()
    pt.render_pass(0, spp)
    _, kernel_ms = pt.kernel_time()
    pt.close()
    return dict(create=statistics.median(create), tree=statistics.median(tree), info=info, kernel=kernel_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--scenes", default="spheres,terrain,room")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        run(args, tmp)


def run(args, tmp):
    table = {"spheres": lambda: (A.HostScene.create_arrays(**scenes.random_spheres(1_000_000, 7)), 1920, 1080, 1),
             "terrain": lambda: (A.HostScene.import_file(workloads.terrain_mesh(16, 56).write(tmp)), 1920, 1080, 3),
             "room": lambda: (A.HostScene.import_file(workloads.room_mesh(3).write(tmp)), 1024, 1024, 7)}
    print(f"library {A.library_path().name}; create = median of 5 after a warm-up create; kernel = one pass of {args.spp} spp after a warm-up pass")
    print("scene     tree    where  create ms  tree ms   nodes   depth  kernel ms")
    for name in args.scenes.split(","):
        hs, W, H, seed = table[name]()
        res = {}
        for device in (False, True):
            r = res[device] = measure(hs, W, H, seed, args.spp, device)
            i = r["info"]
            print(f"{name:9s} {'device' if device else 'host':7s} {i['where']:5d} {r['create']:10.1f} {r['tree']:8.1f} {i['n_nodes']:8d} {i['depth']:6d} {r['kernel']:10.2f}", flush=True)
        h, d = res[False], res[True]
        saved, per_spp = h["create"] - d["create"], (d["kernel"] - h["kernel"]) / args.spp
        even = "never (the device tree renders no slower)" if per_spp <= 0 else f"{saved / per_spp:.0f} spp"
        print(f"{name:9s} create {h['create'] / d['create']:.1f}x shorter, kernel {d['kernel'] / h['kernel']:.2f}x the host tree's; host build + render overtakes at {even}", flush=True)


if __name__ == "__main__":
    main()

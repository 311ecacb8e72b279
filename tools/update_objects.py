#!/usr/bin/env python3
"""amber_hip_pt_update_objects against destroy + create, and what a refit costs the render as objects move.

For config 3's scene (1M spheres) and the 1.04M-triangle terrain, medians of 5 after a warm-up, host clock around calls that end in a
synchronise:  (a) destroy + create(AMBER_PT_FLAG_DEVICE_BUILD);  (b) update REBUILD, all objects;  (c) update REFIT, all objects;
(d) update REFIT, 1 % of the objects.  Then the kernel time (amber_hip_pt_kernel_time) of one pass of --spp samples at the bench's frame
through: a fresh host tree, a fresh device tree, and a device tree refitted after every object moved by a uniform random vector of length
<= 0.25 / 1 / 4 times its own largest box side, each with area_after / area_before and beside the kernel time of a fresh device tree built
on that MOVED scene (the moved scene is another scene to render: only this pair compares trees).  Smallest motion first, every refitted
render in a child process under its own time limit, and the sweep stops at the first step whose kernel time exceeds ten times the fresh
device tree's (a stop rule for a shared machine, not a result).  Writes the table to stdout (profiles/update_objects.txt keeps one run).

    AMBER_AMD_LIB=libamber_hip.so python tools/update_objects.py [--spp 64] [--scenes spheres,terrain]
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import amber_amd as A                                    # noqa: E402
from amber_amd import scenes, workloads                  # noqa: E402

RECORD = np.dtype([("kind", np.uint32), ("material", np.uint32), ("p", np.float32, (12,))])
FRAMES = {"spheres": (1920, 1080, 1), "terrain": (1920, 1080, 3)}
STEPS = (0.25, 1.0, 4.0)


def scene(name):
    kw = scenes.random_spheres(1_000_000, 7) if name == "spheres" else workloads.terrain_mesh(16, 56).arrays()
    hs = A.HostScene.create_arrays(**kw)
    objs, _, lens = hs.flatten()
    return hs, np.frombuffer(objs, dtype=RECORD).copy(), int(lens.first_blade_object), int(lens.n_blades), kw


def moved(rec, factor, seed, first_blade, n_blades):
    """every object but the aperture blades translated by a uniform random vector of length <= factor * its own largest box side"""
    rng = np.random.default_rng(seed)
    out = rec.copy()
    kind, p = out["kind"], out["p"]
    tri = p[:, :9].reshape(-1, 3, 3)
    side = np.where(kind == 0, (tri.max(1) - tri.min(1)).max(1), 2.0 * np.abs(np.where(kind == 1, p[:, 3], p[:, 6])))
    d = rng.normal(size=(len(out), 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    shift = (d * (rng.uniform(0, 1, len(out)) ** (1 / 3) * factor * side)[:, None]).astype(np.float32)
    shift[first_blade:first_blade + n_blades] = 0
    for v in range(3):
        p[:, 3 * v:3 * v + 3] += np.where(((kind == 0) | (v == 0))[:, None], shift, np.float32(0))
    return out


def timed(fn, repeats=5):
    fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def kernel_ms(pt, spp):
    pt.render_pass(0, spp); pt.sync(); pt.clear(); pt.render_pass(0, spp)
    return pt.kernel_time()[1]


def child(name, factor, spp):
    hs, rec, fb, nb, kw = scene(name)
    W, H, seed = FRAMES[name]
    target = moved(rec, factor, 31, fb, nb)
    pt = A.PathTracer(hs, A.Sensor.default(W, H), seed=seed, flags=A.PT_FLAG_DEVICE_BUILD)
    info = pt.update_flat(0, target, A.UPDATE_REFIT)
    ms = kernel_ms(pt, spp)
    pt.close()
    # a fresh device tree on the moved scene (the host model recomputes the triangle normals: the same scene to the last bit or two)
    user = np.delete(np.arange(len(rec)), np.arange(fb, fb + nb))
    pt = A.PathTracer(A.HostScene.create_arrays(**dict(kw, params=target["p"][user])), A.Sensor.default(W, H), seed=seed, flags=A.PT_FLAG_DEVICE_BUILD)
    fresh_ms = kernel_ms(pt, spp)
    pt.close()
    print("RESULT " + json.dumps(dict(kernel=ms, fresh=fresh_ms, ratio=info["area_after"] / info["area_before"], update_ms=info["update_ms"])))


def run(name, spp, limit_s):
    hs, rec, fb, nb, _ = scene(name)
    W, H, seed = FRAMES[name]
    sensor = A.Sensor.default(W, H)
    other = moved(rec, 0.25, 17, fb, nb)
    state = {"pt": A.PathTracer(hs, sensor, seed=seed, flags=A.PT_FLAG_DEVICE_BUILD), "k": 0}

    def recreate():
        state["pt"].close()
        state["pt"] = A.PathTracer(hs, sensor, seed=seed, flags=A.PT_FLAG_DEVICE_BUILD)
        state["pt"].sync()

    def update(mode, lo=0, hi=len(rec)):
        def fn():
            state["k"] += 1
            state["pt"].update_flat(lo, (other if state["k"] % 2 else rec)[lo:hi], mode)
            state["pt"].sync()
        return fn
    n = len(rec)
    a = timed(recreate)
    b = timed(update(A.UPDATE_REBUILD))
    c = timed(update(A.UPDATE_REFIT))
    d = timed(update(A.UPDATE_REFIT, n // 3, n // 3 + n // 100))
    state["pt"].close()
    print(f"{name:8s} {n} objects: destroy + create(DEVICE_BUILD) {a:7.2f} ms | update REBUILD {b:6.2f} ms ({a / b:.1f}x) | update REFIT {c:6.2f} ms ({a / c:.1f}x) | "
          f"REFIT of 1 % {d:6.2f} ms ({a / d:.1f}x)", flush=True)
    fresh = {}
    for device in (False, True):
        pt = A.PathTracer(hs, sensor, seed=seed, flags=A.PT_FLAG_DEVICE_BUILD if device else 0)
        fresh[device] = kernel_ms(pt, spp)
        pt.close()
    print(f"{name:8s} kernel at {spp} spp, {W}x{H}: fresh host tree {fresh[False]:.2f} ms, fresh device tree {fresh[True]:.2f} ms", flush=True)
    for factor in STEPS:
        try:
            p = subprocess.run([sys.executable, __file__, "--child", name, str(factor), "--spp", str(spp)], capture_output=True, text=True, timeout=limit_s)
        except subprocess.TimeoutExpired:
            print(f"{name:8s} motion <= {factor:g} box sides: no result within {limit_s} s; sweep stopped", flush=True)
            break
        if p.returncode != 0:
            print(f"{name:8s} motion <= {factor:g} box sides: the child failed ({p.returncode}); sweep stopped\n{p.stderr[-800:]}", flush=True)
            break
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
        print(f"{name:8s} motion <= {factor:4g} box sides: refitted device tree {r['kernel']:8.2f} ms, fresh device tree on the moved scene {r['fresh']:8.2f} ms "
              f"({r['kernel'] / r['fresh']:.2f}x), area_after / area_before {r['ratio']:.3f}", flush=True)
        if r["kernel"] > 10.0 * r["fresh"]:
            print(f"{name:8s} more than ten times the fresh tree's kernel time: sweep stopped (the stop rule, not a result)", flush=True)
            break


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--scenes", default="spheres,terrain")
    ap.add_argument("--limit", type=int, default=150, help="time limit of one refitted render (a child process), seconds")
    ap.add_argument("--child", nargs=2, metavar=("SCENE", "FACTOR"))
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], float(args.child[1]), args.spp)
    print(f"library {A.library_path().name}; times = median of 5 after a warm-up, each ending in a synchronise; kernel = one pass after a warm-up pass")
    for name in args.scenes.split(","):
        run(name, args.spp, args.limit)


if __name__ == "__main__":
    main()

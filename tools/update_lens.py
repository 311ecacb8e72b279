#!/usr/bin/env python3
"""amber_hip_pt_update_lens against destroy + create, and what the pass after it costs.

For config 3's scene (1M spheres) and the 1.04M-triangle terrain the camera orbits about the world's y axis through a few positions, the last
of them three times as far out -- well outside the scene's bounds, which the old aperture is part of.  A handle created with
AMBER_PT_FLAG_DEVICE_BUILD goes round the positions --repeats + 1 times per mode (the first round is the warm-up).  At every position:
  update_ms of update_lens (AmberUpdateInfo: host wall time of the call, both waits included), REFIT and REBUILD;
  update_ms of update_objects with count = n_blades (the blades just installed, sent again: the same device work) in the same mode;
and, once per position, the kernel time (amber_hip_pt_kernel_time) of one pass of --spp samples after the REFIT and after the REBUILD, beside that
of a fresh handle created on that camera with the host's tree and with the device's.  destroy + create(DEVICE_BUILD) is timed on the first camera
(median of --repeats after a warm-up, to a synchronise).  Acceptance: the median update_ms of update_lens is no more than the median of
update_objects plus that call's run-to-run spread (max - min over its repeats, all positions of the mode together).  A REBUILD whose Morton tree
comes out deeper than the traversal's limit refits instead (AmberUpdateInfo.mode_used); the tool counts those per position.

    AMBER_AMD_LIB=libamber_hip.so python tools/update_lens.py [--spp 16] [--scenes spheres,terrain] [--json FILE]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import amber_amd as A                                    # noqa: E402
from amber_amd import scenes, workloads                  # noqa: E402

RECORD = np.dtype([("kind", np.uint32), ("material", np.uint32), ("p", np.float32, (12,))])
FRAMES = {"spheres": (960, 540, 1), "terrain": (960, 540, 3)}
ORBIT = ((0.0, 1.0), (40.0, 1.0), (80.0, 1.0), (120.0, 3.0))      # degrees about the y axis, distance from the origin as a multiple of the first camera's


def orbit(transform, degrees, scale):
    """the camera turned about the world's y axis, its position scaled"""
    t = np.array(transform, np.float64).reshape(4, 4)
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    r = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]])
    out = r @ t
    out[:3, 3] *= scale
    return [float(x) for x in out.reshape(-1)]


def lens_of(kw, transform):
    """(FlatThinLens, blade records) of kw's lens at `transform`, from the host object model: a scene of one sphere has the same lens and blades"""
    tiny = A.HostScene.create_arrays(np.array([A.api.PRIM_SPHERE], np.uint32), np.zeros(1, np.uint32), np.array([[0, 0, 0, 1]], np.float32), kw["materials"][:1],
                                     transform, kw["focal_length"], kw["focus_distance"], kw["radius"], kw["n_blades"])
    objs, _, lens = tiny.flatten()
    rec = np.frombuffer(objs, dtype=RECORD)[lens.first_blade_object:lens.first_blade_object + lens.n_blades].copy()
    tiny.close()
    return lens, rec


def kernel_ms(pt, spp):
    pt.render_pass(0, spp); pt.sync(); pt.clear(); pt.render_pass(0, spp)
    return pt.kernel_time()[1]


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), spread=max(v) - min(v), n=len(v))


def run(name, spp, repeats):
    kw = scenes.random_spheres(1_000_000, 7) if name == "spheres" else workloads.terrain_mesh(16, 56).arrays()
    W, H, seed = FRAMES[name]
    sensor = A.Sensor.default(W, H)
    hs = A.HostScene.create_arrays(**kw)
    objs, _, lens0 = hs.flatten()
    first, n_blades = int(lens0.first_blade_object), int(lens0.n_blades)
    resident = np.frombuffer(objs, dtype=RECORD)[first:first + n_blades]
    cams = []
    for degrees, scale in ORBIT:
        t = orbit(kw["transform"], degrees, scale)
        lens, rec = lens_of(kw, t)
        lens.first_blade_object = first                              # (the tiny scene's blades come first too; the material is the resident one)
        rec["material"] = resident["material"]
        cams.append(dict(degrees=degrees, scale=scale, transform=t, lens=lens, blades=rec))
    out = dict(scene=name, objects=len(kw["kinds"]) + n_blades, n_blades=n_blades, frame=[W, H, spp], repeats=repeats, positions=[])

    pt = A.PathTracer(hs, sensor, seed=seed, flags=A.PT_FLAG_DEVICE_BUILD)
    t = []
    for k in range(repeats + 1):
        t0 = time.perf_counter()
        pt.close()
        pt = A.PathTracer(hs, sensor, seed=seed, flags=A.PT_FLAG_DEVICE_BUILD)
        pt.sync()
        t.append((time.perf_counter() - t0) * 1e3)
    out["destroy_create_ms"] = stats(t[1:])
    lens_ms = {m: [[] for _ in cams] for m in ("refit", "rebuild")}
    objects_ms = {m: [] for m in ("refit", "rebuild")}
    kernel = {m: [None] * len(cams) for m in ("refit", "rebuild")}
    fallbacks = {m: [0] * len(cams) for m in ("refit", "rebuild")}
    for label, mode in (("refit", A.UPDATE_REFIT), ("rebuild", A.UPDATE_REBUILD)):
        for rep in range(repeats + 1):
            for i, cam in enumerate(cams):
                info = pt.update_lens((cam["lens"], cam["blades"]), mode)
                if info["mode_used"] != mode:                        # a Morton tree deeper than the traversal's limit: the call has refitted instead
                    fallbacks[label][i] += 1
                again = pt.update_flat(first, cam["blades"], mode)
                if rep:
                    lens_ms[label][i].append(info["update_ms"]); objects_ms[label].append(again["update_ms"])
                if rep == repeats:
                    kernel[label][i] = kernel_ms(pt, spp)
    pt.close()
    out["update_objects_n_blades_ms"] = {m: stats(v) for m, v in objects_ms.items()}
    create = out["destroy_create_ms"]["median"]
    print(f"{name:8s} {out['objects']} objects, {n_blades} blades: destroy + create(DEVICE_BUILD) {create:.2f} ms; update_objects of the {n_blades} blades: "
          + "; ".join(f"{m.upper()} {s['median']:.2f} ms (spread {s['spread']:.2f})" for m, s in out["update_objects_n_blades_ms"].items()), flush=True)
    for i, cam in enumerate(cams):
        fresh = {}
        hs_cam = A.HostScene.create_arrays(**dict(kw, transform=cam["transform"]))
        for device in (False, True):
            f = A.PathTracer(hs_cam, sensor, seed=seed, flags=A.PT_FLAG_DEVICE_BUILD if device else 0)
            fresh["device" if device else "host"] = kernel_ms(f, spp)
            f.close()
        hs_cam.close()
        pos = dict(degrees=cam["degrees"], distance=cam["scale"], origin=[float(x) for x in cam["lens"].origin[:]],
                   update_lens_ms={m: stats(lens_ms[m][i]) for m in lens_ms}, rebuilds_that_refitted=fallbacks["rebuild"][i], kernel_ms_after={m: kernel[m][i] for m in kernel}, kernel_ms_fresh=fresh)
        out["positions"].append(pos)
        r, b = pos["update_lens_ms"]["refit"], pos["update_lens_ms"]["rebuild"]
        print(f"{name:8s} {cam['degrees']:5.0f} deg, {cam['scale']:g} x the distance: update_lens REFIT {r['median']:6.2f} ms ({create / r['median']:.1f}x), REBUILD {b['median']:6.2f} ms "
              f"({create / b['median']:.1f}x) | pass of {spp} spp after REFIT {kernel['refit'][i]:7.2f} ms, after REBUILD {kernel['rebuild'][i]:7.2f} ms, "
              f"fresh host tree {fresh['host']:7.2f} ms, fresh device tree {fresh['device']:7.2f} ms"
              + (f" | {fallbacks['rebuild'][i]} of {repeats + 1} REBUILDs refitted instead (Morton tree too deep)" if fallbacks["rebuild"][i] else ""), flush=True)
    out["acceptance"] = {}
    for m in ("refit", "rebuild"):
        ref = out["update_objects_n_blades_ms"][m]
        med = statistics.median([x for per in lens_ms[m] for x in per])
        out["acceptance"][m] = dict(update_lens_median_ms=med, update_objects_median_ms=ref["median"], spread_ms=ref["spread"], within=bool(med <= ref["median"] + ref["spread"]))
        print(f"{name:8s} {m.upper():7s}: update_lens {med:.2f} ms against update_objects(count = n_blades) {ref['median']:.2f} ms + spread {ref['spread']:.2f} ms: "
              f"{'within' if out['acceptance'][m]['within'] else 'NOT within'}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--scenes", default="spheres,terrain")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", help="write the raw figures here")
    args = ap.parse_args()
    print(f"library {A.library_path().name}; update_ms = AmberUpdateInfo.update_ms, medians of {args.repeats} after a warm-up round; kernel = one pass after a warm-up pass")
    results = [run(name, args.spp, args.repeats) for name in args.scenes.split(",")]
    if args.json:
        Path(args.json).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""amber_hip_lt_trace_photons against amber_hip_lt_trace of the same passes on the same handle: the same light paths, traced by the kernels light
tracing had before the vertex sink, which only count and (rarely) splat.

Workloads: the Cornell box at 1024 x 1024 and the 1M-sphere scene (scenes.random_spheres) at 1920 x 1080, --passes passes each, surfaces --surfaces
(default DIFFUSE: PhotonMap::Build's list).  The records go to a device buffer sized by a counting call (torch allocates it); nothing is copied to
the host inside the timed window.  Both calls are synchronous, so each is timed on the host's clock around the call: median of --repeats after a
warm-up call, with the spread (max - min).  The split into trace, sort and gather comes from hipEvents through the lab hook
amber_hip_kat_photon_stage_ms (it makes every launch's gather wait, so it runs in a call of its own); lt_trace's kernel time is not recorded by the
library (its launches are untimed), so its column is the host's clock alone.

    python tools/photons.py [--passes 4] [--repeats 7] [--surfaces 1] [--scenes cornell,spheres] [--out profiles/lt_photons.txt]
    AMBER_AMD_LIB=libamber_hip_NAME.so python tools/photons.py ...      # a measurement build, e.g. make variant NAME=photon_lane DEFS=-DAMBER_PHOTON_CLAIM_PER_LANE=1
"""
import argparse
import os
import statistics
import sys
import time
from pathlib import Path

os.environ.setdefault("AMBER_AMD_LIB", "libamber_hip_lab.so")   # the stage timer is a lab entry point (include/amber_hip_lab.h)
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np                                              # noqa: E402
import torch                                                    # noqa: E402
import amber_amd as A                                           # noqa: E402
from amber_amd import scenes                                    # noqa: E402


def timed(f, repeats):
    """(median ms, spread ms) of f() on the host's clock, after one warm-up call"""
    t = []
    for k in range(repeats + 1):
        t0 = time.perf_counter()
        f()
        if k:
            t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), max(t) - min(t)


def run_scene(name, hs, sensor, passes, surfaces, repeats, say):
    w, h = sensor.width, sensor.height
    pt = A.PathTracer(hs, sensor, seed=13)
    lib = A.load_library()
    import ctypes as C
    info = A.PhotonInfo()
    A.api._check(lib.amber_hip_lt_trace_photons(pt._h, 0, passes, 0, w * h, surfaces, None, 0, C.byref(info), 0))      # the counting call
    need = int(info.n_photons)
    out = torch.empty((max(need, 1), 16), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    got = {}

    def photons():
        got["n"], got["info"] = pt.lt_trace_photons(0, passes, surfaces, out=(out.data_ptr(), need))
    count_ms, count_spread = timed(lambda: lib.amber_hip_lt_trace_photons(pt._h, 0, passes, 0, w * h, surfaces, None, 0, C.byref(info), 0), repeats)
    new_ms, new_spread = timed(photons, repeats)
    splats = {}

    def trace():
        splats["rec"], splats["rays"] = pt.lt_trace(0, passes)
    old_ms, old_spread = timed(trace, repeats)
    stage = (float("nan"),) * 3
    if A.is_lab() and hasattr(lib, "amber_hip_kat_photon_stage_ms"):
        pt.kat_photon_stage_ms()                                       # on, totals reset
        photons()
        stage = pt.kat_photon_stage_ms()
    rec = out[:need].cpu().numpy().view(A.PHOTON_DTYPE).reshape(-1)
    ordered = bool(np.array_equal(np.lexsort((rec["bounce"], rec["path"], rec["sample"])), np.arange(len(rec))))
    pt.close()
    i = got["info"]
    total = sum(stage)
    say(f"{name}, {w} x {h}, {passes} pass(es), surfaces {surfaces}: {i['n_photons']} records ({i['n_photons'] / (w * h * passes):.3f} per path), {i['n_rays']} rays "
        f"(lt_trace: {splats['rays']}, {len(splats['rec'])} splats), {i['n_launches']} launch(es), {i['n_repeats']} repeat(s) in the last call; in key order: {'yes' if ordered else 'NO'}")
    say(f"  median of {repeats} after a warm-up, ms on the host's clock (spread = max - min)")
    say(f"  lt_trace_photons, device buffer  {new_ms:9.3f} (spread {new_spread:.3f})   {i['n_photons'] / new_ms / 1e3:8.2f} M records/s   {i['n_rays'] / new_ms / 1e3:8.2f} M rays/s")
    say(f"  lt_trace_photons, counting call  {count_ms:9.3f} (spread {count_spread:.3f})")
    say(f"  lt_trace                         {old_ms:9.3f} (spread {old_spread:.3f})   {splats['rays'] / old_ms / 1e3:8.2f} M rays/s   photons / lt_trace = {new_ms / old_ms:.3f}")
    say(f"  by hipEvents: trace {stage[0]:.3f}   sort {stage[1]:.3f}   gather {stage[2]:.3f}"
        + (f"   -- shares {100 * stage[0] / total:.1f} % / {100 * stage[1] / total:.1f} % / {100 * stage[2] / total:.1f} %" if total == total and total > 0 else ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--surfaces", type=int, default=A.PHOTON_DIFFUSE)
    ap.add_argument("--scenes", default="cornell,spheres")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"library {A.library_path().name}")
    for scene in args.scenes.split(","):
        if scene == "cornell":
            run_scene("Cornell box", A.HostScene.cornell_box(), A.Sensor.default(1024, 1024), args.passes, args.surfaces, args.repeats, say)
        elif scene == "spheres":
            run_scene("1M spheres", A.HostScene.create_arrays(**scenes.random_spheres(1_000_000, 7)), A.Sensor.default(1920, 1080), args.passes, args.surfaces, args.repeats, say)
        else:
            raise SystemExit(f"unknown scene {scene}")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

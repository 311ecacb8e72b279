#!/usr/bin/env python3
"""amber_hip_pt_aov_pass against amber_hip_pt_render_pass of the same sample count on the same handle.

Two workloads: the Cornell box at 1024 x 1024 (engine TWO_PHASE) and the 1M-sphere scene at 1920 x 1080 (engine BVH).  Each call is timed between two
events on the handle's stream (the call enqueues only; the events bracket everything it enqueues), the best of --repeats after a warm-up call.  An AOV
pass casts one ray per path and sums eight numbers per pixel; a render pass traces the whole path and reduces its records -- the expectation is only
that the first costs less than the second.  The tool also checks that the coverage sum of the pass is plausible (0 < hits <= paths).

    AMBER_AMD_LIB=libamber_hip.so python tools/aov.py [--spp 8] [--repeats 10] [--out profiles/aov.txt]
"""
import argparse
import sys
from pathlib import Path

import torch
torch.cuda.init()                                               # (torch's runtime up before the engine's library)

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import amber_amd as A                                           # noqa: E402
from amber_amd import scenes                                    # noqa: E402


def best_events(pt, ext, f, repeats):
    """best time in ms between two events around f() on the handle's stream, after one warm-up call"""
    t = []
    with torch.cuda.stream(ext):
        f(); pt.sync()
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ext); f(); e1.record(ext)
            pt.sync(); e1.synchronize()
            t.append(e0.elapsed_time(e1))
    return min(t)


def run(name, hs, w, h, engine, spp, repeats, say):
    dev = torch.device("cuda", 0)
    pt = A.PathTracer(hs, A.Sensor.default(w, h), seed=7, engine=engine)
    ext = torch.cuda.ExternalStream(pt.stream(), device=dev)
    pt.render_pass(0, spp); pt.sync()                           # the handle's first launch measures the record density: not timed
    t_render = best_events(pt, ext, lambda: pt.render_pass(0, spp), repeats)
    t_aov = best_events(pt, ext, lambda: pt.aov_pass(0, spp), repeats)
    pt.aov_clear(); pt.aov_pass(0, spp)
    hits = float(pt.aov_download()[..., 7].astype("float64").sum())
    pt.close()
    assert 0 < hits <= w * h * spp, hits
    say(f"{name}, {w} x {h}, {spp} spp, best of {repeats} after a warm-up, ms between events on the handle's stream")
    say(f"  render_pass {t_render:9.3f}   aov_pass {t_aov:9.3f}   aov_pass / render_pass = {t_aov / t_render:.3f}   "
        f"({hits / (w * h * spp):.3f} of the eye rays hit; aov_pass below render_pass: {'yes' if t_aov < t_render else 'NO'})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", help="write the report here as well")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"tools/aov.py: library {A.library_path().name}, {torch.cuda.get_device_name(0)}")
    run("Cornell box, engine TWO_PHASE", A.HostScene.cornell_box(), 1024, 1024, A.ENGINE_TWO_PHASE, args.spp, args.repeats, say)
    run("1M spheres, engine BVH", A.HostScene.create_arrays(**scenes.random_spheres(1_000_000, 7)), 1920, 1080, A.ENGINE_BVH, args.spp, args.repeats, say)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

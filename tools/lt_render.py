#!/usr/bin/env python3
"""amber_hip_lt_render_pass against amber_hip_lt_trace plus a host accumulation of the same passes, on one handle.

Workloads: the `lights` scene of the tests (wide aperture; its sensor enlarged --scale times so that what comes through the aperture lands on it) at
1024 x 768 and the Cornell box at 1024 x 1024, --passes passes each; and synthetic loads of 1e6 and 1e7 records through the lab hook
amber_hip_kat_lt_accumulate, which alone puts the ordering and the ordered sum under load (real scenes splat rarely).

Both calls are synchronous, so each is timed on the host's clock around the call (framebuffer cleared outside the window): median of --repeats after a
warm-up call, with the spread (max - min).  The host accumulation is numpy's (np.add.at per pass over lt_trace's list), a stand-in for the C++ loop at the
end of HipLightTracing::Render, which --adapter times itself.  The split into trace, sort and sum comes from hipEvents: amber_hip_pt_kernel_time for the
trace launches, amber_hip_kat_lt_stage_ms (lab build; it makes every accumulation wait, so it runs in a pass of its own) for the other two.

    python tools/lt_render.py [--passes 8] [--repeats 9] [--scale 4] [--out profiles/lt_render_pass.txt]
    AMBER_AMD_LIB=libamber_hip.so python tools/lt_render.py --adapter [--passes 64] [--repeats 9]     # `--algorithm lt` through HipLightTracing::Render
"""
import argparse
import os
import statistics
import sys
import time
from pathlib import Path

os.environ.setdefault("AMBER_AMD_LIB", "libamber_hip_lab.so")   # the hook and the stage timer are lab entry points (include/amber_hip_lab.h)
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np                                              # noqa: E402
import amber_amd as A                                           # noqa: E402

LIGHTS = dict(
    materials=[(4, (30.0, 20.0, 10.0), 0.0), (0, (0.7, 0.6, 0.5), 0.0), (2, (0.8, 0.8, 0.8), 0.0), (3, (1.0, 1.0, 1.0), 1.5), (4, (5.0, 5.0, 9.0), 0.0)],
    objects=[
        (2, 0, [0.0, 1.5, 0.0, 0.0, -1.0, 0.0, 0.6]), (0, 4, [-1.0, 1.4, -1.0, -1.0, 1.4, 1.0, -0.5, 1.4, 0.0]), (1, 0, [1.2, 0.8, 0.0, 0.15]),
        (3, 4, [-1.4, -0.5, 0.5, 0.0, 1.0, 0.0, 0.1, 0.6]), (0, 1, [-3, -1, -3, 3, -1, 3, 3, -1, -3]), (0, 1, [-3, -1, -3, -3, -1, 3, 3, -1, 3]),
        (1, 2, [0.7, -0.6, -0.3, 0.4]), (1, 3, [0.0, -0.5, 0.8, 0.45]),
    ],
    transform=[1, 0, 0, 0, 0, 1, 0, 0.2, 0, 0, 1, 2.6, 0, 0, 0, 1], focal_length=0.05, focus_distance=2.6, radius=0.45, n_blades=5,
)


def sensor_of(width, height, scale):
    return A.Sensor(width, height, np.float32(0.036 * scale), np.float32(0.036 / width * height * scale))


def timed(f, repeats, before=None):
    """(median ms, spread ms) of f() on the host's clock, after one warm-up call; before() runs outside the window"""
    t = []
    for k in range(repeats + 1):
        if before:
            before()
        t0 = time.perf_counter()
        f()
        if k:
            t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), max(t) - min(t)


def host_accumulate(rec, width, height):
    total = np.zeros((width * height, 3), np.float32)
    if len(rec):
        cuts = np.flatnonzero(np.diff(rec["sample"])) + 1
        for part in np.split(rec, cuts):
            image = np.zeros((width * height, 3), np.float32)
            np.add.at(image, part["pixel"], part["rgb"])               # in list order: (path, bounce) within the pass
            total += image
    return total


def run_scene(name, hs, sensor, passes, repeats, say):
    w, h = sensor.width, sensor.height
    pt = A.PathTracer(hs, sensor, seed=13)

    def clear():
        pt.clear(); pt.sync()
    new_ms, new_spread = timed(lambda: pt.lt_render_pass(0, passes), repeats, clear)
    clear()
    info = pt.lt_render_pass(0, passes)
    launches, trace_ms = pt.kernel_time()
    img_new, rays_new = pt.download()
    got = {}

    def old():
        got["rec"], got["rays"] = pt.lt_trace(0, passes, capacity=max(1 << 16, info["n_splats"]))
        got["img"] = host_accumulate(got["rec"], w, h)
    old_ms, old_spread = timed(old, repeats)
    trace_only_ms, _ = timed(lambda: pt.lt_trace(0, passes, capacity=max(1 << 16, info["n_splats"])), repeats)
    same = np.array_equal(img_new.reshape(-1, 3).view(np.uint32), got["img"].view(np.uint32)) and rays_new == got["rays"]
    sort_ms = sum_ms = float("nan")
    if A.is_lab():
        pt.kat_lt_stage_ms()                                           # on, totals reset
        clear(); pt.lt_render_pass(0, passes)
        sort_ms, sum_ms = pt.kat_lt_stage_ms()
    pt.close()
    say(f"{name}, {w} x {h}, {passes} passes: {info['n_splats']} records, {info['n_rays']} rays, {info['n_launches']} launch(es), longest run {info['longest_run']}; "
        f"median of {repeats} after a warm-up, ms on the host's clock (spread = max - min)")
    say(f"  lt_render_pass                   {new_ms:9.3f} (spread {new_spread:.3f})")
    say(f"  lt_trace + host accumulation     {old_ms:9.3f} (spread {old_spread:.3f}), of which lt_trace {trace_only_ms:.3f}")
    say(f"  by hipEvents: trace {trace_ms:.3f} ({launches} launch(es))   sort {sort_ms:.3f}   sum {sum_ms:.3f}"
        f"   -- the same bits and rays as the host accumulation: {'yes' if same else 'NO'}")


def run_synthetic(n, say, repeats):
    w, h, passes = 1024, 768, 8
    rng = np.random.default_rng(n)
    rec = np.zeros(n, A.SPLAT_DTYPE)
    rec["path"] = rng.integers(0, w * h, n); rec["sample"] = rng.integers(0, passes, n); rec["bounce"] = rng.integers(1, 9, n)
    rec["pixel"] = rng.integers(0, w * h, n); rec["rgb"] = rng.random((n, 3), np.float32)
    pt = A.PathTracer(A.HostScene.create(**LIGHTS), A.Sensor.default(w, h), seed=13)
    ms, spread = timed(lambda: pt.kat_lt_accumulate(rec), repeats)
    pt.kat_lt_stage_ms()
    pt.kat_lt_accumulate(rec)
    sort_ms, sum_ms = pt.kat_lt_stage_ms()
    pt.close()
    say(f"synthetic, {n} records over {w} x {h}, {passes} passes, uniformly random pixels: the hook (upload of {n * 32 >> 20} MiB included) "
        f"{ms:.3f} ms (spread {spread:.3f}); by hipEvents: sort {sort_ms:.3f}   sum {sum_ms:.3f}")


def run_adapter(passes, repeats, scale, say):
    hs = A.HostScene.create(**LIGHTS)
    for label, sensor in ((f"sensor x {scale}", sensor_of(1024, 768, scale)), ("default sensor", A.Sensor.default(1024, 768))):
        out = {}

        def f():
            out["img"], out["st"] = hs.render(sensor, passes, seed=13, samples_per_launch=16, algorithm="lt")
        ms, spread = timed(f, repeats)
        say(f"adapter, lights 1024 x 768, {label}, {passes} passes in launches of 16: wall {ms:.3f} ms (spread {spread:.3f}), median of {repeats}; "
            f"{out['st']['rays']} rays, image sum {float(out['img'].astype(np.float64).sum()):.9g}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--scale", type=float, default=4.0)
    ap.add_argument("--adapter", action="store_true")
    ap.add_argument("--skip-large", action="store_true", help="leave the 1e7-record load out")
    ap.add_argument("--out", help="append the report here as well")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"tools/lt_render.py{' --adapter' if args.adapter else ''}: library {A.library_path().name}")
    if args.adapter:
        run_adapter(args.passes or 64, args.repeats, args.scale, say)
    else:
        run_scene(f"lights (sensor x {args.scale:g})", A.HostScene.create(**LIGHTS), sensor_of(1024, 768, args.scale), args.passes or 8, args.repeats, say)
        run_scene("Cornell box", A.HostScene.cornell_box(), A.Sensor.default(1024, 1024), args.passes or 8, args.repeats, say)
        run_synthetic(1_000_000, say, args.repeats)
        if not args.skip_large:
            run_synthetic(10_000_000, say, max(7, args.repeats // 2))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""amber_hip_pt_temporal: what the call costs beside the calls it stands next to, and what a reprojected history does to the error of a few samples.

(a) Cost at 1920 x 1080 on the Cornell box and the 1M-sphere scene (engine BVH: the only engine whose handles take amber_hip_pt_update_lens), RGBA8
    into a device tensor.  Every time is between two events on the handle's stream (the calls enqueue only), the best of --repeats after a warm-up.
      temporal(levels = 0)   temporal_kernel + the output stage, beside resolve() (the output stage alone) and beside a device-to-device copy of
                             184 bytes per pixel: the 44 the kernel reads of this frame, the 64 of one previous record it gathers at the least,
                             the 76 it writes
      temporal(levels = 5)   beside denoise(levels = 5) on the same handle: the five levels and the output stage are the same kernels over the same
                             bytes, so the difference is temporal_kernel against denoise_prepare_kernel
    each with the lens unchanged (one tap) and with a moved lens (four taps): for the latter amber_hip_pt_update_lens alternates between two cameras
    0.3 degrees of orbit apart in front of every timed call, outside the events.
(b) Error.  A 16-frame orbit of the Cornell camera about the world's y axis through the origin, which is the box's centre, 0.25 degrees per frame
    (by geometry, not measured: the centre stays where it is in the image, a point on the box's front or back face moves by about one pixel), through
    update_lens at 512 x 512, once with one lt_render_pass per frame and once with 4 spp of render_pass per frame (fresh sample indices every frame).
    Per frame: the RMSE over all channels against a --ref-spp frame of the same lens rendered on a second handle with another seed, of the raw
    frame, of denoise(), of temporal(levels = 0) and of temporal(levels = 5) (two handles run the same orbit, one per setting: a call moves the
    history), and the share of pixels whose history was kept (length > 1 after the call).
The parameters are the defaults, which nobody has tuned.

    AMBER_AMD_LIB=libamber_hip.so python tools/temporal.py [--repeats 20] [--out profiles/temporal.txt]
"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch
torch.cuda.init()                                               # (torch's runtime up before the engine's library)

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import amber_amd as A                                           # noqa: E402
from amber_amd import scenes                                    # noqa: E402

LEVELS = 5
COPY_BYTES = 44 + 64 + 76


def orbit(hs, degrees):
    """(lens, blade records) of the scene's camera turned about the world's y axis through the origin: the pair amber_hip_pt_update_lens takes"""
    objs, _, lens = hs.flatten()
    t = np.radians(degrees)
    R = np.array([[np.cos(t), 0, np.sin(t)], [0, 1, 0], [-np.sin(t), 0, np.cos(t)]])
    rec = np.frombuffer(objs, dtype=A.api._RECORD)
    blades = rec[lens.first_blade_object:lens.first_blade_object + lens.n_blades].copy()
    p = blades["p"].astype(np.float64).reshape(-1, 4, 3)                        # v0 v1 v2 normal
    blades["p"] = (p @ R.T).reshape(-1, 12).astype(np.float32)
    new = type(lens).from_buffer_copy(lens)
    g = R @ np.array(list(lens.global_), np.float64).reshape(3, 3)
    o = R @ np.array(list(lens.origin), np.float64)
    for i in range(3):
        new.origin[i] = o[i]
    for i in range(9):
        new.global_[i], new.local_[i] = g.reshape(9)[i], np.linalg.inv(g).reshape(9)[i]
    return new, blades


def best_events(pt, ext, f, repeats, before=None):
    """best time in ms between two events around f() on the handle's stream, after one warm-up call; before() runs in front of every call, outside"""
    t = []
    with torch.cuda.stream(ext):
        if before:
            before()
        f(); pt.sync()
        for _ in range(repeats):
            if before:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ext); f(); e1.record(ext)
            pt.sync(); e1.synchronize()
            t.append(e0.elapsed_time(e1))
    return min(t)


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def cost(name, hs, w, h, repeats, say):
    dev = torch.device("cuda", 0)
    pt = A.PathTracer(hs, A.Sensor.default(w, h), seed=7, engine=A.ENGINE_BVH)
    ext = torch.cuda.ExternalStream(pt.stream(), device=dev)
    cams, turn = [orbit(hs, 0.0), orbit(hs, 0.3)], [0]

    def move():
        turn[0] ^= 1
        pt.update_lens(cams[turn[0]])
    pt.render_pass(0, 4); pt.aov_pass(0, 4); pt.sync()
    with torch.cuda.stream(ext):
        rgba = torch.empty((h, w, 4), dtype=torch.uint8, device=dev)
        src, dst = torch.zeros(w * h * COPY_BYTES, dtype=torch.uint8, device=dev), torch.empty(w * h * COPY_BYTES, dtype=torch.uint8, device=dev)
        pt.sync()
    t_out = best_events(pt, ext, lambda: pt.resolve(4, A.RESOLVE_RGBA8, out=rgba), repeats)
    t_copy = best_events(pt, ext, lambda: dst.copy_(src, non_blocking=True), repeats)
    t_den = best_events(pt, ext, lambda: pt.denoise(4, levels=LEVELS, format=A.RESOLVE_RGBA8, out=rgba), repeats)
    t = {}
    for levels in (0, LEVELS):
        call = lambda: pt.temporal(4, levels=levels, format=A.RESOLVE_RGBA8, out=rgba)
        pt.temporal_reset(); call()
        t[levels, "same"] = best_events(pt, ext, call, repeats)
        t[levels, "moved"] = best_events(pt, ext, call, repeats, before=move)
    kept = float((pt.history_download()[..., 3] > 1).mean())
    pt.close()
    say(f"{name}, {w} x {h}, engine BVH, RGBA8 to a device tensor; best of {repeats} after a warm-up, ms between events on the handle's stream")
    say(f"  temporal(levels = 0): lens unchanged {t[0, 'same']:.4f}   lens moved {t[0, 'moved']:.4f}   beside resolve {t_out:.4f}   and a device copy of {COPY_BYTES} bytes per pixel "
        f"({w * h * COPY_BYTES / 1e6:.0f} MB, twice that of traffic) {t_copy:.4f}")
    say(f"    so temporal_kernel alone (the call minus the output stage): lens unchanged {t[0, 'same'] - t_out:.4f}   lens moved {t[0, 'moved'] - t_out:.4f}")
    say(f"  temporal(levels = {LEVELS}): lens unchanged {t[LEVELS, 'same']:.4f}   lens moved {t[LEVELS, 'moved']:.4f}   beside denoise(levels = {LEVELS}) {t_den:.4f}"
        f"   differences {t[LEVELS, 'same'] - t_den:+.4f} / {t[LEVELS, 'moved'] - t_den:+.4f} (temporal_kernel against denoise_prepare_kernel)")
    say(f"  (share of pixels whose history was kept in the last moved-lens call: {kept:.3f})")


def error(hs, light_traced, frames, ref_spp, say):
    w = h = 512
    spp = 1 if light_traced else 4
    sensor = A.Sensor.default(w, h)
    render = lambda pt, first, n: (pt.lt_render_pass if light_traced else pt.render_pass)(first, n)
    plain, filtered = (A.PathTracer(hs, sensor, seed=7, engine=A.ENGINE_BVH) for _ in range(2))
    ref = A.PathTracer(hs, sensor, seed=1234, engine=A.ENGINE_BVH)
    what = f"one lt_render_pass per frame" if light_traced else f"{spp} spp of render_pass per frame"
    say(f"Cornell box, {w} x {h}, {frames}-frame orbit of 0.25 degrees per frame, {what}; RMSE against {ref_spp} {'passes' if light_traced else 'spp'} of the same lens (another seed)")
    say("  frame        raw    denoise   temporal(levels=0)   temporal(levels=5)   history kept")
    sums = np.zeros(4)
    for f in range(frames):
        cam = orbit(hs, 0.25 * f)
        out = []
        for pt in (plain, filtered, ref):
            if f:
                pt.update_lens(cam)
            pt.clear()
        render(ref, 0, ref_spp)
        truth = ref.resolve(ref_spp, A.RESOLVE_MEAN_F32)
        for pt in (plain, filtered):
            render(pt, f * spp, spp); pt.aov_clear(); pt.aov_pass(f * spp, spp)
        raw = plain.resolve(spp, A.RESOLVE_MEAN_F32)
        den = plain.denoise(spp, levels=LEVELS, format=A.RESOLVE_MEAN_F32)
        t0 = plain.temporal(spp, levels=0, format=A.RESOLVE_MEAN_F32)
        t5 = filtered.temporal(spp, levels=LEVELS, format=A.RESOLVE_MEAN_F32)
        kept = float((plain.history_download()[..., 3] > 1).mean())
        e = np.array([rmse(raw, truth), rmse(den, truth), rmse(t0, truth), rmse(t5, truth)])
        sums += e
        say(f"  {f:5d}  {e[0]:9.6f}  {e[1]:9.6f}  {e[2]:9.6f} ({e[2] / e[0]:.3f})  {e[3]:9.6f} ({e[3] / e[0]:.3f})  {kept:.3f}")
    m = sums / frames
    say(f"  mean   {m[0]:9.6f}  {m[1]:9.6f}  {m[2]:9.6f} ({m[2] / m[0]:.3f})  {m[3]:9.6f} ({m[3] / m[0]:.3f})")
    for pt in (plain, filtered, ref):
        pt.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--out", help="write the report here as well")
    ap.add_argument("--skip-spheres", action="store_true", help="the Cornell box only")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"tools/temporal.py: library {A.library_path().name}, {torch.cuda.get_device_name(0)}; default parameters (levels 5, max_history 32, k 4 / 100 / 10 / 0.25)")
    cost("Cornell box", A.HostScene.cornell_box(), 1920, 1080, args.repeats, say)
    if not args.skip_spheres:
        cost("1M spheres", A.HostScene.create_arrays(**scenes.random_spheres(1_000_000, 7)), 1920, 1080, args.repeats, say)
    for light_traced in (True, False):
        error(A.HostScene.cornell_box(), light_traced, args.frames, args.ref_spp, say)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""amber_hip_pt_denoise: what the call costs, beside the samples it would have to replace, and what it does to the error of a 4-spp frame.

Three workloads: the Cornell box at 1024 x 1024 and 1920 x 1080, the 1M-sphere scene at 1920 x 1080 (engine BVH); levels = 5 and the default
parameters, RGBA8 into a device tensor.  Every time is between two events on the handle's stream (the calls enqueue only), the best of --repeats
after a warm-up call.
  whole call     prepare kernel + 5 level kernels + the output stage: 7 launches
  stages         the call cannot be bracketed from inside, so the stages are differences of whole calls: level i (i >= 1) = call(levels = i + 1) -
                 call(levels = i) -- the first i levels of the two are the same work -- the output stage = resolve() of the same format on the same
                 handle (the same kernel over the same bytes), and prepare + level 0 = call(levels = 1) - output stage
  beside it      render_pass of 1, 4 and 16 samples on the same handle: what the filter must undercut to pay
                 a device-to-device copy of levels * 56 + 44 bytes per pixel, the bytes the call must move at least (a level reads 44 and writes 12,
                 prepare reads 44: the write of prepare, the output stage and every re-read of a tap are on top)
  RMSE           of the 4-spp mean and of its denoised image (MEAN_F32) against a 1024-spp mean of the same handle (samples 4 .. 1027: independent
                 of the frame that is filtered), over all channels; the same with k_color = 0 (the guides alone), because a low-sample frame of a
                 scene whose light is found by chance is a few very bright pixels in black, which the colour stop keeps apart

    AMBER_AMD_LIB=libamber_hip.so python tools/denoise.py [--repeats 20] [--out profiles/denoise.txt]
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

LEVELS, SPP, REF_SPP = 5, 4, 1024


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


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def run(name, hs, w, h, engine, repeats, say):
    dev = torch.device("cuda", 0)
    n_pixels = w * h
    pt = A.PathTracer(hs, A.Sensor.default(w, h), seed=7, engine=engine)
    ext = torch.cuda.ExternalStream(pt.stream(), device=dev)
    # ---- the error of the 4-spp frame before and after
    pt.render_pass(0, SPP); pt.aov_pass(0, SPP)
    noisy = pt.resolve(SPP, A.RESOLVE_MEAN_F32)
    clean = pt.denoise(SPP, levels=LEVELS, format=A.RESOLVE_MEAN_F32)
    guided = pt.denoise(SPP, levels=LEVELS, k_color=0.0, format=A.RESOLVE_MEAN_F32)
    hit_share = float(pt.aov_download()[..., 7].astype(np.float64).sum()) / (n_pixels * SPP)
    pt.clear(); pt.render_pass(SPP, REF_SPP)
    ref = pt.resolve(REF_SPP, A.RESOLVE_MEAN_F32)
    changed = int((noisy.view(np.uint32) != clean.view(np.uint32)).sum())
    finite = np.isfinite(ref).all() and np.isfinite(noisy).all() and np.isfinite(clean).all()
    e_noisy, e_clean, e_guided = rmse(noisy, ref), rmse(clean, ref), rmse(guided, ref)
    # ---- times
    pt.clear(); pt.render_pass(0, SPP); pt.sync()
    with torch.cuda.stream(ext):
        rgba = torch.empty((h, w, 4), dtype=torch.uint8, device=dev)
        moved = n_pixels * (LEVELS * 56 + 44)
        src, dst = torch.zeros(moved, dtype=torch.uint8, device=dev), torch.empty(moved, dtype=torch.uint8, device=dev)
        pt.sync()
    call = [best_events(pt, ext, lambda: pt.denoise(SPP, levels=L, format=A.RESOLVE_RGBA8, out=rgba), repeats) for L in range(1, LEVELS + 1)]
    t_out = best_events(pt, ext, lambda: pt.resolve(SPP, A.RESOLVE_RGBA8, out=rgba), repeats)
    t_copy = best_events(pt, ext, lambda: dst.copy_(src, non_blocking=True), repeats)
    t_render = {n: best_events(pt, ext, lambda: pt.render_pass(0, n), repeats) for n in (1, 4, 16)}
    pt.close()
    whole = call[-1]
    say(f"{name}, {w} x {h}, levels {LEVELS}, default parameters, RGBA8 to a device tensor; best of {repeats} after a warm-up, ms between events on the handle's stream")
    say(f"  whole call ({LEVELS + 2} launches)   {whole:9.4f}")
    say(f"  stages (differences, see the tool's text): prepare + level 0 {call[0] - t_out:.4f}   " +
        "   ".join(f"level {i} {call[i] - call[i - 1]:.4f}" for i in range(1, LEVELS)) + f"   output stage (resolve alone) {t_out:.4f}")
    say("  render_pass on the same handle: " + "   ".join(f"{n} spp {t:.3f} (call / it = {whole / t:.3f})" for n, t in t_render.items()) +
        f"   -- the call is {'below' if whole < t_render[1] else 'NOT below'} one sample, {'below' if whole < t_render[4] else 'NOT below'} four")
    say(f"  device copy of {LEVELS * 56 + 44} bytes per pixel ({moved / 1e6:.0f} MB, twice that of traffic) {t_copy:.4f}   call / copy = {whole / t_copy:.2f}")
    say(f"  RMSE against the {REF_SPP}-spp mean: {SPP}-spp mean {e_noisy:.6g}   denoised {e_clean:.6g} ({e_clean / e_noisy:.3f} of it)   with k_color = 0, the guides alone, "
        f"{e_guided:.6g} ({e_guided / e_noisy:.3f})   bits changed by the default call: {changed} of {noisy.size}"
        f"   ({hit_share:.3f} of the eye rays hit; all values finite: {'yes' if finite else 'NO'})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", help="write the report here as well")
    ap.add_argument("--skip-spheres", action="store_true", help="the two Cornell frames only")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"tools/denoise.py: library {A.library_path().name}, {torch.cuda.get_device_name(0)}")
    run("Cornell box", A.HostScene.cornell_box(), 1024, 1024, A.ENGINE_AUTO, args.repeats, say)
    run("Cornell box", A.HostScene.cornell_box(), 1920, 1080, A.ENGINE_AUTO, args.repeats, say)
    if not args.skip_spheres:
        run("1M spheres, engine BVH", A.HostScene.create_arrays(**scenes.random_spheres(1_000_000, 7)), 1920, 1080, A.ENGINE_BVH, args.repeats, say)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

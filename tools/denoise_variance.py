#!/usr/bin/env python3
"""amber_hip_pt_denoise_variance and amber_hip_pt_render_batch: what they cost, beside amber_hip_pt_denoise and the samples, and what the filter does
to the error of a 4-spp frame that amber_hip_pt_denoise returns unchanged.

Three workloads: the Cornell box at 1024 x 1024 and 1920 x 1080, the 1M-sphere scene at 1920 x 1080 (engine BVH); levels = 5 and the default
parameters, RGBA8 into a device tensor.  The frame is four batches of one sample (render_batch(s, 1), s = 0 .. 3) plus aov_pass(0, 4).  Every time is
between two events on the handle's stream (the calls enqueue only), the best of --repeats after a warm-up call.
  whole call     guide prepare + moments prepare + variance kernel (var_radius 3: 49 taps) + 5 level kernels + the output stage: 9 launches
  stages         differences of whole calls, as tools/denoise.py: level i (i >= 1) = call(levels = i + 1) - call(levels = i), the output stage =
                 resolve() of the same format, the three kernels in front + level 0 = call(levels = 1) - output stage; and the pool alone =
                 call(levels = 1, var_radius = 3) - call(levels = 1, var_radius = 0)
  beside it      amber_hip_pt_denoise at the same size and level count on the same handle in the same run; render_pass of 1 and 4 samples
  batches        four render_batch(s, 1) against one render_pass(0, 4): a launch has a fixed cost, and a batch adds a memset and the fold kernel, so
                 the ratio is well above 1 -- reported plainly
  RMSE           against a 1024-spp mean of other samples (4 .. 1027), over all channels: the 4-spp mean, amber_hip_pt_denoise with its defaults, the
                 new call with its defaults; and the new call with var_radius = 0 (the pixel's own variance: a black pixel next to a firefly has none)

    AMBER_AMD_LIB=libamber_hip.so python tools/denoise_variance.py [--repeats 20] [--out profiles/denoise_variance.txt]
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
from denoise import best_events, rmse                           # noqa: E402  (tools/denoise.py)

LEVELS, SPP, REF_SPP = 5, 4, 1024


def batches(pt):
    for s in range(SPP):
        pt.render_batch(s, 1)


def run(name, hs, w, h, engine, repeats, say):
    dev = torch.device("cuda", 0)
    pt = A.PathTracer(hs, A.Sensor.default(w, h), seed=7, engine=engine)
    ext = torch.cuda.ExternalStream(pt.stream(), device=dev)
    # ---- the error of the 4-spp frame before and after
    batches(pt); pt.aov_pass(0, SPP)
    noisy = pt.resolve(SPP, A.RESOLVE_MEAN_F32)
    plain = pt.denoise(SPP, levels=LEVELS, format=A.RESOLVE_MEAN_F32)
    guided = pt.denoise_variance(SPP, levels=LEVELS, format=A.RESOLVE_MEAN_F32)
    own = pt.denoise_variance(SPP, levels=LEVELS, var_radius=0, format=A.RESOLVE_MEAN_F32)
    moments = pt.moments_download()
    lit = float((moments[..., 1] > 0).mean())
    pt.clear(); pt.render_pass(SPP, REF_SPP)
    ref = pt.resolve(REF_SPP, A.RESOLVE_MEAN_F32)
    finite = all(np.isfinite(a).all() for a in (ref, noisy, plain, guided, own))
    e_noisy, e_plain, e_guided, e_own = rmse(noisy, ref), rmse(plain, ref), rmse(guided, ref), rmse(own, ref)
    # ---- times
    pt.clear(); pt.moments_clear(); batches(pt); pt.sync()
    with torch.cuda.stream(ext):
        rgba = torch.empty((h, w, 4), dtype=torch.uint8, device=dev)
        pt.sync()
    call = [best_events(pt, ext, lambda: pt.denoise_variance(SPP, levels=L, format=A.RESOLVE_RGBA8, out=rgba), repeats) for L in range(1, LEVELS + 1)]
    t_own = best_events(pt, ext, lambda: pt.denoise_variance(SPP, levels=1, var_radius=0, format=A.RESOLVE_RGBA8, out=rgba), repeats)
    t_plain = best_events(pt, ext, lambda: pt.denoise(SPP, levels=LEVELS, format=A.RESOLVE_RGBA8, out=rgba), repeats)
    t_out = best_events(pt, ext, lambda: pt.resolve(SPP, A.RESOLVE_RGBA8, out=rgba), repeats)
    t_render = {n: best_events(pt, ext, lambda: pt.render_pass(0, n), repeats) for n in (1, 4)}
    t_batches = best_events(pt, ext, lambda: batches(pt), repeats)
    pt.close()
    whole = call[-1]
    say(f"{name}, {w} x {h}, levels {LEVELS}, default parameters, RGBA8 to a device tensor; best of {repeats} after a warm-up, ms between events on the handle's stream")
    say(f"  amber_hip_pt_denoise_variance, whole call ({LEVELS + 4} launches)   {whole:9.4f}   amber_hip_pt_denoise ({LEVELS + 2} launches) {t_plain:.4f}   ratio {whole / t_plain:.3f}")
    say(f"  stages (differences, see the tool's text): prepare x 2 + variance (var_radius 3) + level 0 {call[0] - t_out:.4f} (of which the pool against var_radius 0: {call[0] - t_own:.4f})   " +
        "   ".join(f"level {i} {call[i] - call[i - 1]:.4f}" for i in range(1, LEVELS)) + f"   output stage (resolve alone) {t_out:.4f}")
    say("  render_pass on the same handle: " + "   ".join(f"{n} spp {t:.3f} (call / it = {whole / t:.3f})" for n, t in t_render.items()) +
        f"   -- the call is {'below' if whole < t_render[1] else 'NOT below'} one sample, {'below' if whole < t_render[4] else 'NOT below'} four")
    say(f"  four render_batch(s, 1) {t_batches:.4f}   one render_pass(0, 4) {t_render[4]:.4f}   ratio {t_batches / t_render[4]:.2f}   (four render_pass(s, 1) would be {4 * t_render[1]:.4f})")
    say(f"  RMSE against the {REF_SPP}-spp mean: {SPP}-spp mean {e_noisy:.6g}   amber_hip_pt_denoise {e_plain:.6g} ({e_plain / e_noisy:.3f} of it)   "
        f"amber_hip_pt_denoise_variance {e_guided:.6g} ({e_guided / e_noisy:.3f})   with var_radius = 0 {e_own:.6g} ({e_own / e_noisy:.3f})"
        f"   ({lit:.4f} of the pixels saw light in some batch; all values finite: {'yes' if finite else 'NO'})")


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
    say(f"tools/denoise_variance.py: library {A.library_path().name}, {torch.cuda.get_device_name(0)}")
    run("Cornell box", A.HostScene.cornell_box(), 1024, 1024, A.ENGINE_AUTO, args.repeats, say)
    run("Cornell box", A.HostScene.cornell_box(), 1920, 1080, A.ENGINE_AUTO, args.repeats, say)
    if not args.skip_spheres:
        run("1M spheres, engine BVH", A.HostScene.create_arrays(**scenes.random_spheres(1_000_000, 7)), 1920, 1080, A.ENGINE_BVH, args.repeats, say)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

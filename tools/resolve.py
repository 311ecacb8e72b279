#!/usr/bin/env python3
"""amber_hip_pt_resolve against the round trip it replaces: download() + the host's tone map.

The Cornell box at 1024 x 1024 and 1920 x 1080, one handle per frame size, one pass of --spp samples; then, each the best of --repeats after a
warm-up call, host wall time from the call until the result is there:
  (a) the parent's path: download() (12 bytes per pixel over the bus, synchronises), then amber.tonemap(sum / n) on the host -- both parts and the sum;
  (b) resolve(RGB8) with AMBER_RESOLVE_HOST: kernel, 3 bytes per pixel over the bus, synchronise;
  (c) resolve(RGBA8) into a device tensor on the handle's stream, from the call to the end of sync();
  (d) the floor of (c): a device-to-device hipMemcpyAsync (torch's Tensor.copy_ between contiguous tensors of one device) on the same stream, timed
      the same way.  (c) reads 12 and writes 4 bytes per pixel; a copy of S bytes reads S and writes S, so the copy of the same traffic is
      8 bytes per pixel.  The copy of 16 bytes per pixel (32 of traffic) is printed beside it.
For (c) and (d) the time between two events on the stream is printed as well: the host figures of calls this short are mostly launch and
synchronise.  The tool asserts that (a) and (b) give the same bytes.

    AMBER_AMD_LIB=libamber_hip.so python tools/resolve.py [--spp 16] [--repeats 20] [--out profiles/resolve.txt]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch
torch.cuda.init()                                               # (torch's runtime up before the engine's library)

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import amber_amd as A                                           # noqa: E402

FRAMES = ((1024, 1024), (1920, 1080))


def best(f, repeats):
    """(best wall ms, last result) of f() over `repeats` calls after one warm-up call"""
    f()
    t, r = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = f()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t), r


def best_events(ext, f, repeats):
    """best time in ms between two events around f() on the stream ext (f enqueues only)"""
    t = []
    with torch.cuda.stream(ext):
        f()
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ext); f(); e1.record(ext)
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
    return min(t)


def run(w, h, spp, repeats, say):
    dev = torch.device("cuda", 0)
    pt = A.PathTracer(A.HostScene.cornell_box(), A.Sensor.default(w, h), seed=7)
    pt.render_pass(0, spp); pt.sync()
    n_pixels = w * h

    t_down, (total, _) = best(pt.download, repeats)
    t_tone, ldr = best(lambda: A.tonemap(total / np.float32(spp)), max(3, repeats // 4))       # single-threaded powf: seconds in all at this size
    t_host, rgb = best(lambda: pt.resolve(spp, A.RESOLVE_RGB8), repeats)
    assert np.array_equal(rgb, ldr), "resolve(RGB8) and download() + tonemap() differ"

    ext = torch.cuda.ExternalStream(pt.stream(), device=dev)
    with torch.cuda.stream(ext):
        rgba = torch.empty((h, w, 4), dtype=torch.uint8, device=dev)
        src8, dst8 = torch.zeros(n_pixels * 8, dtype=torch.uint8, device=dev), torch.empty(n_pixels * 8, dtype=torch.uint8, device=dev)
        src16, dst16 = torch.zeros(n_pixels * 16, dtype=torch.uint8, device=dev), torch.empty(n_pixels * 16, dtype=torch.uint8, device=dev)
        pt.sync()

        def resolve_device():
            pt.resolve(spp, A.RESOLVE_RGBA8, out=rgba)

        def synced(f):
            def g():
                f(); pt.sync()
            return g
        t_dev, _ = best(synced(resolve_device), repeats)
        t_copy8, _ = best(synced(lambda: dst8.copy_(src8, non_blocking=True)), repeats)
        t_copy16, _ = best(synced(lambda: dst16.copy_(src16, non_blocking=True)), repeats)
    assert np.array_equal(rgba.cpu().numpy()[..., :3], ldr) and bool((rgba[..., 3] == 255).all())
    e_dev = best_events(ext, resolve_device, repeats)
    e_copy8 = best_events(ext, lambda: dst8.copy_(src8, non_blocking=True), repeats)
    e_copy16 = best_events(ext, lambda: dst16.copy_(src16, non_blocking=True), repeats)
    pt.close()

    a = t_down + t_tone
    say(f"{w} x {h}, {spp} spp, best of {repeats} after a warm-up, ms")
    say(f"  (a) download() + amber.tonemap(sum / n)        {a:10.3f}   = download {t_down:.3f} ({12 * n_pixels / 1e6:.1f} MB) + tone map on the host {t_tone:.3f}")
    say(f"  (b) resolve(RGB8), AMBER_RESOLVE_HOST          {t_host:10.3f}   ({3 * n_pixels / 1e6:.1f} MB over the bus; bytes equal to (a): yes)   (a) / (b) = {a / t_host:.1f}")
    say(f"  (c) resolve(RGBA8) to a device tensor + sync   {t_dev:10.3f}   between events {e_dev:.4f}   ({16 * n_pixels / 1e6:.1f} MB of traffic)   (a) / (c) = {a / t_dev:.0f}")
    say(f"  (d) device copy of 8 bytes per pixel + sync    {t_copy8:10.3f}   between events {e_copy8:.4f}   (the same traffic)   (c) / (d) = {t_dev / t_copy8:.2f}, between events {e_dev / e_copy8:.2f}")
    say(f"      device copy of 16 bytes per pixel + sync   {t_copy16:10.3f}   between events {e_copy16:.4f}   (twice the traffic)  (c) / it  = {t_dev / t_copy16:.2f}, between events {e_dev / e_copy16:.2f}")
    say(f"  (c) faster than (a): {'yes' if t_dev < a else 'NO'}; (c) within twice (d): {'yes' if t_dev <= 2 * t_copy8 else 'NO'} by the host clock, "
        f"{'yes' if e_dev <= 2 * e_copy8 else 'NO'} between events")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", help="write the report here as well")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"tools/resolve.py: library {A.library_path().name}, {torch.cuda.get_device_name(0)}; host wall time unless it says 'between events'")
    for w, h in FRAMES:
        run(w, h, args.spp, args.repeats, say)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

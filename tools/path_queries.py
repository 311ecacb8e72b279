#!/usr/bin/env python3
"""amber_hip_pt_trace_paths against amber_hip_pt_render_pass of the same number of paths on the same handle.

Two workloads: the Cornell box (engine TWO_PHASE) and the 1M-sphere scene (engine BVH).  The rays are the eye rays of a 1024 x 1024 frame (sample 0 of
every pixel, from the lab's kat_eye), gathered once as positions and directions and packed once into AmberPathRay records in device memory; each ray
takes --spp samples, so a call traces as many paths as render_pass(0, spp) of that frame.  Each call is timed between two events on the handle's
stream (the call enqueues only), the best of --repeats after a warm-up call.  Reported: paths per second of each, the casts of the query, and the
ratio to render_pass.

The kernel refills idle lanes per ray from one counter.  Its A/B baseline -- one thread per ray, finished lanes waiting for their wave -- was a
second build of the library measured by this tool in a process of its own; it lost and its macro arm was deleted (profiles/path_queries.txt holds
that run, EXPERIMENTS.md the reason).  --also LABEL=LIBRARY measures a further lab build next to the product's kernel the same way, for the next A/B:
    make -C amber_amd/csrc variant NAME=claim256 DEFS=-DAMBER_PATH_CLAIM=256u
    python tools/path_queries.py --also claim256=libamber_hip_claim256.so

    python tools/path_queries.py [--spp 8] [--repeats 5] [--also LABEL=LIBRARY ...] [--out profiles/path_queries.txt]
"""
import argparse
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
FORMS = [("refill", "libamber_hip_lab.so")]
W = H = 1024


def child(form, spp, repeats):
    import numpy as np
    import torch
    torch.cuda.init()                                           # (torch's runtime up before the engine's library)
    sys.path.insert(0, str(ROOT))
    import amber_amd as A
    from amber_amd import scenes

    def best_events(pt, ext, f):
        t = []
        with torch.cuda.stream(ext):
            f(); pt.sync()
            for _ in range(repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(ext); f(); e1.record(ext)
                pt.sync(); e1.synchronize()
                t.append(e0.elapsed_time(e1))
        return min(t)

    assert A.is_lab(), "the eye rays come from the lab's kat_eye"
    dev = torch.device("cuda", 0)
    lib = A.load_library()
    print(f"form {form}: library {A.library_path().name}, {torch.cuda.get_device_name(0)}", flush=True)
    for name, make, engine in (("Cornell box, engine TWO_PHASE", A.HostScene.cornell_box, A.ENGINE_TWO_PHASE),
                               ("1M spheres, engine BVH", lambda: A.HostScene.create_arrays(**scenes.random_spheres(1_000_000, 7)), A.ENGINE_BVH)):
        pt = A.PathTracer(make(), A.Sensor.default(W, H), seed=7, engine=engine)
        ext = torch.cuda.ExternalStream(pt.stream(), device=dev)
        n = W * H
        pixel = np.arange(n, dtype=np.uint32)
        eye = pt.kat_eye(pixel, np.zeros(n, np.uint32))
        packed = np.zeros(n, A.api._PATH_RAY)
        packed["origin"], packed["dir"], packed["weight"] = eye[:, 0:3], eye[:, 3:6], eye[:, 6:7]
        packed["rng_state"] = A.sampler_states(7, pixel, np.zeros(n))
        rays = torch.from_numpy(packed.view(np.uint8).reshape(n, 64)).to(dev)
        out = torch.empty((n, 8), dtype=torch.float32, device=dev)
        pt.render_pass(0, spp); pt.sync()                       # the handle's first launch measures the record density: not timed
        t_render = best_events(pt, ext, lambda: pt.render_pass(0, spp))

        def query():
            assert lib.amber_hip_pt_trace_paths(pt._h, n, rays.data_ptr(), out.data_ptr(), spp, 0, 0) == 0
        t_query = best_events(pt, ext, query)
        casts = int(out[:, 3].contiguous().view(torch.int32).cpu().numpy().view(np.uint32).astype(np.uint64).sum())
        pt.close()
        paths = n * spp
        print(f"{name}, {n} rays x {spp} samples = {paths} paths, best of {repeats} after a warm-up, ms between events on the handle's stream\n"
              f"  {form:6s} trace_paths {t_query:9.3f} ms  {paths / t_query / 1e3:9.1f} M paths/s  {casts / t_query / 1e3:9.1f} M casts/s ({casts / paths:.2f} casts a path)\n"
              f"         render_pass {t_render:9.3f} ms  {paths / t_render / 1e3:9.1f} M paths/s   trace_paths / render_pass = {t_query / t_render:.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", help="write the report here as well")
    ap.add_argument("--also", action="append", default=[], metavar="LABEL=LIBRARY", help="a further lab build of the library, measured the same way")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.spp, args.repeats)
        return
    lines = ["tools/path_queries.py"]
    print(lines[0], flush=True)
    for form, libname in FORMS + [tuple(x.split("=", 1)) for x in args.also]:
        if not (ROOT / "amber_amd" / "lib" / libname).exists():
            text = f"form {form}: {libname} is not there (see the head of this tool)"
        else:
            p = subprocess.run([sys.executable, __file__, "--child", form, "--spp", str(args.spp), "--repeats", str(args.repeats)],
                               env=dict(os.environ, AMBER_AMD_LIB=libname), capture_output=True, text=True)
            text = p.stdout.rstrip() if p.returncode == 0 else f"form {form}: failed\n{p.stderr[-2000:]}"
        print(text, flush=True)
        lines.append(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

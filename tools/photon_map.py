#!/usr/bin/env python3
"""amber_hip_pm_build / amber_hip_pm_gather next to the calls that feed them, on the same handle.

Workloads: the Cornell box at 1024 x 1024 and the 1M-sphere scene (scenes.random_spheres) at 1920 x 1080.  Photons: one DIFFUSE pass of
amber_hip_lt_trace_photons into a device buffer.  Queries: sample 0 of every pixel's eye ray (the lab hook kat_eye) through cast_rays; the hits on
Lambertian and Phong surfaces become queries (pos, normal, object of the hit, dir_out = -ray direction, weight 1), in pixel order, in a device buffer.
k = 1024, the reference's constant (algorithm_sppm.cc:202).  Three radii: r1024 is the radius at which the median query of a 4096-query sample has
1024 photons in radius (found by two steps of r <- r * sqrt(1024 / median N): N grows with r^2 on a surface); the runs use 0.5, 1.0 and 1.6 times
r1024 -- from almost no query capped to most (how many at 1.0 depends on how evenly the scene's photons lie) -- with cell_size = radius.

Printed per radius: build ms (hipEvents, and the host's clock around the call) next to the lt_trace_photons ms of the same photons; gather ms
(hipEvents through amber_hip_kat_pm_stage_ms; median of --repeats) next to one sample of render_pass on the same handle (amber_hip_pt_kernel_time);
the share of queries on the slow path (n_in_radius > k); candidates visited per photon used (the photons in the visited cells, counted on the host
from the map's own grid for a sample of the queries, over n_used).

    python tools/photon_map.py [--repeats 3] [--scenes cornell,spheres] [--k 1024] [--out profiles/photon_map.txt]
"""
import argparse
import os
import statistics
import sys
import time
from pathlib import Path

os.environ.setdefault("AMBER_AMD_LIB", "libamber_hip_lab.so")   # the eye rays and the stage timer are lab entry points (include/amber_hip_lab.h)
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np                                              # noqa: E402
import torch                                                    # noqa: E402
import amber_amd as A                                           # noqa: E402
from amber_amd import scenes                                    # noqa: E402

F = np.float32


def candidates_visited(info, photons_pos, q_pos, radius):
    """Photons in the cells each query visits: the contract's cell range (binary32, as the kernel forms it) over a 3-D prefix sum of the cell counts."""
    lo, dims, inv = np.asarray(info["lo"], F), np.asarray(info["dims"], np.int64), F(1) / F(info["cell_size"])
    cell = np.floor((photons_pos - lo) * inv).astype(np.int64)
    counts = np.bincount((cell[:, 2] * dims[1] + cell[:, 1]) * dims[0] + cell[:, 0], minlength=int(dims.prod())).reshape(dims[2], dims[1], dims[0])
    pre = np.zeros((dims[2] + 1, dims[1] + 1, dims[0] + 1), np.int64)
    pre[1:, 1:, 1:] = counts.cumsum(0).cumsum(1).cumsum(2)
    top = (dims - 1).astype(F)
    flo, fhi = np.floor(((q_pos - F(radius)) - lo) * inv), np.floor(((q_pos + F(radius)) - lo) * inv)
    empty = ((fhi < 0) | (flo > top)).any(axis=1)
    c0 = np.clip(flo, 0, top).astype(np.int64)
    c1 = np.clip(fhi, 0, top).astype(np.int64) + 1
    x0, y0, z0, x1, y1, z1 = c0[:, 0], c0[:, 1], c0[:, 2], c1[:, 0], c1[:, 1], c1[:, 2]
    box = (pre[z1, y1, x1] - pre[z0, y1, x1] - pre[z1, y0, x1] - pre[z1, y1, x0] + pre[z0, y0, x1] + pre[z0, y1, x0] + pre[z1, y0, x0] - pre[z0, y0, x0])
    return np.where(empty, 0, box)


def run_scene(name, hs, sensor, k, repeats, say):
    w, h = sensor.width, sensor.height
    pt = A.PathTracer(hs, sensor, seed=13)
    objs, mats, _ = hs.flatten()
    kinds = np.array([m.kind for m in mats])[np.frombuffer(objs, dtype=A.api._RECORD)["material"]]       # material kind of every object
    # ---- photons: one DIFFUSE pass, into a device buffer
    _, count = pt.lt_trace_photons(0, 1, A.PHOTON_DIFFUSE, out=(None, 0))
    n_ph = count["n_photons"]
    photons = torch.empty((max(n_ph, 1), 16), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    t = []
    for _ in range(repeats + 1):
        t0 = time.perf_counter()
        pt.lt_trace_photons(0, 1, A.PHOTON_DIFFUSE, out=(photons.data_ptr(), n_ph))
        t.append((time.perf_counter() - t0) * 1e3)
    photons_ms = statistics.median(t[1:])
    photons = photons[:n_ph]
    ph_pos = photons[:, 0:3].cpu().numpy()
    # ---- queries: the first diffuse hit of every pixel's eye ray
    pix = np.arange(w * h, dtype=np.uint32)
    eye = pt.kat_eye(pix, np.zeros(len(pix), np.uint32))
    obj, _, pos, nrm = pt.cast_rays(eye[:, 0:3] + eye[:, 3:6] * F(1e-3), eye[:, 3:6])
    keep = (obj >= 0) & (kinds[np.clip(obj, 0, None)] <= A.api.MAT_PHONG)
    q = np.zeros(int(keep.sum()), A.GATHER_QUERY_DTYPE)
    q["pos"], q["normal"], q["object"], q["dir_out"], q["weight"] = pos[keep], nrm[keep], obj[keep], -eye[keep, 3:6], (1, 1, 1)
    n_q = len(q)
    # ---- one sample of render_pass on the same handle
    pt.render_pass(0, 1)
    pt.sync()
    pt.clear()
    pt.render_pass(0, 1)
    render_ms = pt.kernel_time()[1]
    say(f"{name}, {w} x {h}: {n_ph} photons of one DIFFUSE pass (lt_trace_photons {photons_ms:.2f} ms), {n_q} queries ({100 * n_q / (w * h):.1f} % of the eye rays end on a diffuse surface), "
        f"k = {k}; one sample of render_pass {render_ms:.2f} ms")
    # ---- r1024: the radius at which the median query has k photons in radius
    extent = float((ph_pos.max(axis=0) - ph_pos.min(axis=0)).max())
    sample = q[np.random.default_rng(1).choice(n_q, min(4096, n_q), replace=False)]
    r = extent * 0.02
    for _ in range(2):
        pt.pm_build(photons, r)
        sample["radius"] = r
        med = float(np.median(pt.pm_gather(sample, k=0, raw=True)["n_in_radius"]))
        r *= (k / max(med, 1.0)) ** 0.5
    say(f"  r1024 = {r:.5g} ({r / extent:.4f} of the photons' extent)")
    pt.kat_pm_stage_ms()                                                 # the timing on, totals reset
    dq = torch.from_numpy(q.view(np.float32).reshape(-1, 16).copy()).cuda()
    out = torch.empty((n_q, 8), dtype=torch.float32, device="cuda")
    say("  radius/r1024   cells (doublings)          build ms: events / host   gather ms (spread)   gather / render_pass   slow path   in radius: median   candidates / used")
    for scale in (0.5, 1.0, 1.6):
        radius = F(r * scale)
        dq[:, 3] = float(radius)
        torch.cuda.synchronize()
        host = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            info = pt.pm_build(photons, float(radius))
            host.append((time.perf_counter() - t0) * 1e3)
        build_ev = pt.kat_pm_stage_ms()[0] / repeats
        g = []
        for i in range(repeats + 1):
            pt.pm_gather(dq, k=k, out=out)
            ms = pt.kat_pm_stage_ms()[1]
            if i:
                g.append(ms)
        res = out.cpu().numpy().view(A.GATHER_RESULT_DTYPE).reshape(-1)
        slow = float((res["n_in_radius"] > k).mean())
        pick = np.random.default_rng(2).choice(n_q, min(65536, n_q), replace=False)
        visited = candidates_visited(info, ph_pos, q["pos"][pick], radius)
        used = res["n_used"][pick].astype(np.int64)
        gather_ms = statistics.median(g)
        say(f"  {scale:11.1f}   {str(info['dims']):18s} ({info['n_doublings']})   {build_ev:9.2f} / {statistics.median(host):7.2f}   {gather_ms:10.2f} ({max(g) - min(g):.2f})   "
            f"{gather_ms / render_ms:18.2f}   {100 * slow:7.1f} %   {int(np.median(res['n_in_radius'])):15d}   {visited.sum() / max(used.sum(), 1):14.2f}")
        say(f"                build / lt_trace_photons = {build_ev / photons_ms:.2f}; {n_q / gather_ms / 1e3:.2f} M queries/s; largest cell {info['max_cell_count']} photons")
    pt.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--k", type=int, default=1024)
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
            run_scene("Cornell box", A.HostScene.cornell_box(), A.Sensor.default(1024, 1024), args.k, args.repeats, say)
        elif scene == "spheres":
            run_scene("1M spheres", A.HostScene.create_arrays(**scenes.random_spheres(1_000_000, 7)), A.Sensor.default(1920, 1080), args.k, args.repeats, say)
        else:
            raise SystemExit(f"unknown scene {scene}")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""How fast are amber_hip_pt_cast_rays and amber_hip_pt_occluded?  (EXPERIMENTS.md, ray queries.)  For the 1M-sphere scene and the terrain mesh,
with a host-built and a device-built tree each: the engine's own eye and secondary rays (amber_hip_kat_eye / amber_hip_kat_trace of random pixels:
exact eye rays, then from every hit point towards the next), 2^20 of them walked 4 times per launch, through
    cast_rays, occluded with t_max = INFINITY, occluded with t_max = half the scene diagonal   (device pointers, events on the handle's stream)
    and the lab's traversal-only kernel, amber_hip_kat_traversal_rate, at the same 5 waves per SIMD and refill threshold of 16.
Every answer is checked: cast_rays against the traversal-only kernel's hits, occluded against cast_rays' distances.  Prints Mrays/s and writes
profiles/ray_queries.json.
    python tools/ray_queries.py [--scenes spheres,terrain] [--out profiles/ray_queries.json]"""
import argparse, json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R)
os.environ.setdefault("AMBER_AMD_LIB", "libamber_hip_lab.so")   # the yardstick and the ray generators are lab entry points (include/amber_hip_lab.h)
import numpy as np
import torch
torch.cuda.init()                                               # (torch's runtime up before the engine's library)
import amber_amd as A
from amber_amd import scenes
from amber_amd import workloads as WL

N_UNIQUE, REPEATS, WAVES, REFILL = 1 << 20, 4, 5, 16


def path_rays(pt, W, H, n_paths, rng, maxb=8):
    px, sm = rng.integers(0, W * H, n_paths).astype(np.uint32), rng.integers(0, 256, n_paths).astype(np.uint32)
    eye = pt.kat_eye(px, sm)
    rec, casts = pt.kat_trace(px, sm, maxb)
    obj, pos = rec[:, :, 0].view(np.int32), rec[:, :, 2:5].view(np.float32)
    org, dirs = [eye[:, 0:3]], [eye[:, 3:6]]
    for k in range(1, maxb):
        ok = (obj[:, k - 1] >= 0) & (obj[:, k] >= 0) & (casts > k)
        o = pos[ok, k - 1]; d = pos[ok, k] - o
        ln = np.linalg.norm(d, axis=1, keepdims=True); keep = ln[:, 0] > 1e-6
        org.append(o[keep]); dirs.append((d[keep] / ln[keep]).astype(np.float32))
    org, dirs = np.concatenate(org), np.concatenate(dirs)
    perm = rng.permutation(len(org))                            # mixed bounce depths per wave, like the render
    return np.ascontiguousarray(org[perm], np.float32), np.ascontiguousarray(dirs[perm], np.float32)


def best_ms(ext, call, reps=5):
    times = []
    with torch.cuda.stream(ext):
        for k in range(reps + 1):                               # a warm-up first
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ext); rc = call(); e1.record(ext); e1.synchronize()
            assert rc == 0, A.load_library().amber_hip_last_error()
            if k: times.append(e0.elapsed_time(e1))
    return min(times)


def measure(name, hs, W, H, device_build):
    dev = torch.device("cuda", 0)
    lib = A.load_library()
    pt = A.PathTracer(hs, A.Sensor.default(W, H), seed=1, flags=A.PT_FLAG_DEVICE_BUILD if device_build else 0)
    info = pt.build_info()
    rng = np.random.default_rng(3)
    org, dirs = path_rays(pt, W, H, 420_000, rng)
    while len(org) < N_UNIQUE:
        o2, d2 = path_rays(pt, W, H, 420_000, rng)
        org, dirs = np.concatenate([org, o2]), np.concatenate([dirs, d2])
    org, dirs = np.ascontiguousarray(org[:N_UNIQUE]), np.ascontiguousarray(dirs[:N_UNIQUE])
    n = N_UNIQUE * REPEATS
    yard = []
    for _ in range(3):
        yo, yt, ms = pt.kat_traversal_rate(org, dirs, waves=WAVES, refill_min=REFILL, repeats=REPEATS)
        yard.append(ms)
    objs, _, _ = hs.flatten()
    anchors = np.frombuffer(objs, dtype=A.api._RECORD)["p"][:, :3]
    half_diag = 0.5 * float(np.linalg.norm(np.nanmax(anchors, 0) - np.nanmin(anchors, 0)))
    packed = np.zeros((N_UNIQUE, 8), np.float32); packed[:, 0:3], packed[:, 3], packed[:, 4:7] = org, np.inf, dirs
    rays = torch.from_numpy(np.tile(packed, (REPEATS, 1))).to(dev)
    rays_half = rays.clone(); rays_half[:, 3] = half_diag
    hits = torch.empty((n, 8), dtype=torch.float32, device=dev)
    occ = torch.empty(n, dtype=torch.uint8, device=dev)
    ext = torch.cuda.ExternalStream(pt.stream(), device=dev)
    torch.cuda.synchronize()
    ms = {"traversal_only": min(yard)}
    ms["cast_rays"] = best_ms(ext, lambda: lib.amber_hip_pt_cast_rays(pt._h, n, rays.data_ptr(), hits.data_ptr(), 0))
    h = hits[:N_UNIQUE].cpu().numpy()
    got_obj, got_t = h[:, 1].copy().view(np.int32), h[:, 0].copy()
    hit = yo >= 0
    assert np.array_equal(got_obj, yo) and np.array_equal(got_t[hit].view(np.uint32), yt[hit].view(np.uint32)), "cast_rays differs from the traversal-only kernel"
    ms["occluded_inf"] = best_ms(ext, lambda: lib.amber_hip_pt_occluded(pt._h, n, rays.data_ptr(), occ.data_ptr(), 0))
    assert np.array_equal(occ[:N_UNIQUE].cpu().numpy() != 0, hit), "occluded(INFINITY) differs from cast_rays"
    ms["occluded_half_diag"] = best_ms(ext, lambda: lib.amber_hip_pt_occluded(pt._h, n, rays_half.data_ptr(), occ.data_ptr(), 0))
    with np.errstate(invalid="ignore"):
        assert np.array_equal(occ[:N_UNIQUE].cpu().numpy() != 0, hit & (got_t <= np.float32(half_diag))), "occluded(half diagonal) differs from cast_rays"
    pt.close()
    row = dict(scene=name, tree="device" if device_build else "host", n_nodes=info["n_nodes"], depth=info["depth"], rays=n, hit_fraction=float(hit.mean()),
               half_diagonal=half_diag, ms=ms, mrays_per_s={k: n / v / 1e3 for k, v in ms.items()},
               cast_over_traversal_only=ms["cast_rays"] / ms["traversal_only"], any_hit_over_closest_hit=ms["occluded_inf"] / ms["cast_rays"])
    print("%-8s %-6s tree (%d nodes, depth %d), %d rays, %.0f %% hit:" % (name, row["tree"], info["n_nodes"], info["depth"], n, 100 * row["hit_fraction"]))
    for k in ("traversal_only", "cast_rays", "occluded_inf", "occluded_half_diag"):
        print("    %-20s %8.3f ms  %8.0f Mrays/s" % (k, ms[k], row["mrays_per_s"][k]))
    print("    cast_rays / traversal-only %.3f, occluded(INFINITY) / cast_rays %.3f" % (row["cast_over_traversal_only"], row["any_hit_over_closest_hit"]), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="spheres,terrain")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "ray_queries.json"))
    args = ap.parse_args()
    table = {"spheres": lambda: (A.HostScene.create_arrays(**scenes.random_spheres(1_000_000, 7)), 1920, 1080),
             "terrain": lambda: (A.HostScene.create_arrays(**WL.terrain_mesh(16, 56).arrays()), 1920, 1080)}
    rows = []
    for name in args.scenes.split(","):
        hs, W, H = table[name]()
        for device_build in (False, True):
            rows.append(measure(name, hs, W, H, device_build))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(waves_per_simd=WAVES, refill_min=REFILL, unique_rays=N_UNIQUE, repeats=REPEATS, rows=rows), f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

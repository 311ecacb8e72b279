"""A/B of two lab builds of the library in ONE process for the kernels behind the queries, light tracing, photons and engine BVH's schedulers: interleaved
pairs after two warm-up rounds, the order swapped every pair (the shape of ab_lib.py --pairs, which covers config 2).

   python tools/ab_device_fold.py [PAIRS] [cornell,spheres,lab] [--parent A.so] [--new B.so] [--out FILE]

A.so (default libamber_hip_parent.so: `make variant NAME=parent` in a checkout of the parent commit, copied into amber_amd/lib) against B.so (default
libamber_hip_lab.so).  ms on the host's clock around call + sync (light tracing, photons, signatures: the whole call, host work included), or the handle's
kernel time (render_pass).  Per figure: both sides' runs, medians, the parent's own spread and whether the new median lies inside it.  `lab`: the lab and
signature kernels and the light tracers of the other engines, on small loads."""
import json, os, statistics, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R)
import numpy as np
import torch
import amber_amd.api as api
import amber_amd as A
from amber_amd import scenes

def opt(flag, default):
    return sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default
PARENT, NEW = opt("--parent", "libamber_hip_parent.so"), opt("--new", "libamber_hip_lab.so")
plain = [a for k, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and not sys.argv[k - 1].startswith("--")]
PAIRS = int(plain[0]) if plain else 12
which = set(plain[1].split(",")) if len(plain) > 1 else {"cornell", "spheres"}
dev = torch.device("cuda", 0)
libs = {}
for path in (PARENT, NEW):
    api._lib = None; api._LIB_PATH = api._ROOT / "lib" / path
    libs[path] = A.load_library()
out_lines = []

def say(s):
    print(s, flush=True); out_lines.append(s)

def use(path):
    api._lib = libs[path]
    return libs[path]

def pairs(label, fns):
    """fns: {lib: callable returning ms}"""
    for _ in range(2):
        for p in (PARENT, NEW): fns[p]()
    res = {PARENT: [], NEW: []}
    for k in range(PAIRS):
        for p in ((PARENT, NEW) if k % 2 == 0 else (NEW, PARENT)):
            res[p].append(fns[p]())
    a, b = res[PARENT], res[NEW]
    med_a, med_b = statistics.median(a), statistics.median(b)
    verdict = "inside the parent's spread" if min(a) <= med_b <= max(a) else ("FASTER than every parent run" if med_b < min(a) else "SLOWER than every parent run")
    say(f"{label}\n    parent " + " ".join("%9.3f" % x for x in a) + f"   median {med_a:9.3f}   spread {min(a):9.3f} .. {max(a):9.3f} ({max(a) - min(a):.3f})\n"
        f"    new    " + " ".join("%9.3f" % x for x in b) + f"   median {med_b:9.3f}   {verdict}")

def host_ms(pt, f):
    pt.sync(); t0 = time.perf_counter(); f(); pt.sync(); return (time.perf_counter() - t0) * 1e3

def make(path, hs_kw, sensor, **kw):
    use(path)
    hs = hs_kw() 
    return hs, A.PathTracer(hs, A.Sensor.default(*sensor), **kw)

def render_fn(path, pt, spp):
    def f():
        use(path); pt.clear(); pt.render_pass(0, spp); pt.sync(); return pt.kernel_time()[1]
    return f

def path_query_fn(path, pt, W, H, spp):
    lib = use(path)
    n = W * H
    pixel = np.arange(n, dtype=np.uint32)
    eye = pt.kat_eye(pixel, np.zeros(n, np.uint32))
    packed = np.zeros(n, api._PATH_RAY)
    packed["origin"], packed["dir"], packed["weight"] = eye[:, 0:3], eye[:, 3:6], eye[:, 6:7]
    packed["rng_state"] = A.sampler_states(7, pixel, np.zeros(n))
    rays = torch.from_numpy(packed.view(np.uint8).reshape(n, 64)).to(dev)
    out = torch.empty((n, 8), dtype=torch.float32, device=dev)
    def call():
        assert lib.amber_hip_pt_trace_paths(pt._h, n, rays.data_ptr(), out.data_ptr(), spp, 0, 0) == 0
    def f():
        use(path); return host_ms(pt, call)
    f.keep = (rays, out)
    return f

def ray_query_fns(path, pt, W, H):
    lib = use(path)
    n = W * H
    pixel = np.arange(n, dtype=np.uint32)
    eye = pt.kat_eye(pixel, np.zeros(n, np.uint32))
    packed = np.zeros(n, api._RAY)
    packed["origin"], packed["dir"], packed["t_max"] = eye[:, 0:3], eye[:, 3:6], np.inf
    rays = torch.from_numpy(packed.view(np.uint8).reshape(n, -1)).to(dev)
    hits = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    occ = torch.empty((n,), dtype=torch.uint8, device=dev)
    def cast():
        assert lib.amber_hip_pt_cast_rays(pt._h, n, rays.data_ptr(), hits.data_ptr(), 0) == 0
    def occl():
        assert lib.amber_hip_pt_occluded(pt._h, n, rays.data_ptr(), occ.data_ptr(), 0) == 0
    def fc():
        use(path); return host_ms(pt, cast)
    def fo():
        use(path); return host_ms(pt, occl)
    fc.keep = (rays, hits, occ)
    return fc, fo

def lt_fn(path, pt, passes):
    def f():
        use(path); return host_ms(pt, lambda: pt.lt_trace(0, passes, capacity=1 << 20))
    return f

def photon_fn(path, pt, passes):
    def f():
        use(path); return host_ms(pt, lambda: pt.lt_trace_photons(0, passes))
    return f

say(f"{torch.cuda.get_device_name(0)}; {PAIRS} pairs after two warm-up rounds, parent = {PARENT} (the parent commit, -DAMBER_LAB), new = {NEW}")
if "cornell" in which:
    W = H = 1024
    for engine_name, flags, tag in (("ENGINE_TWO_PHASE", 0, "path_query_kernel<TWO_PHASE>"), ("ENGINE_LIST", 0, "path_query_kernel<LIST>"), ("ENGINE_BVH", 0, "path_query_kernel<BVH>")):
        h = {p: make(p, A.HostScene.cornell_box, (W, H), seed=7, engine=getattr(A, engine_name)) for p in (PARENT, NEW)}
        pairs(f"trace_paths, Cornell 1024^2 eye rays x 4 samples, {tag}: ms on the host's clock", {p: path_query_fn(p, h[p][1], W, H, 4) for p in h})
        for p in h: use(p); h[p][1].close()
    for flags, tag in ((0, "pt_megakernel<TWO_PHASE, light>"), (A.PT_FLAG_BVH_ITEMS, "pt_bvh_megakernel<light>")):
        kw = dict(seed=7) if not flags else dict(seed=7, engine=A.ENGINE_BVH, flags=flags)
        h = {p: make(p, A.HostScene.cornell_box, (W, H), **kw) for p in (PARENT, NEW)}
        pairs(f"lt_trace, Cornell 1024^2, 4 passes, {tag}: ms on the host's clock (the whole call)", {p: lt_fn(p, h[p][1], 4) for p in h})
        pairs(f"lt_trace_photons, Cornell 1024^2, 2 passes, DIFFUSE, {tag} with the vertex sink: ms on the host's clock (the whole call)", {p: photon_fn(p, h[p][1], 2) for p in h})
        for p in h: use(p); h[p][1].close()
    h = {p: make(p, A.HostScene.cornell_box, (W, H), seed=7, engine=A.ENGINE_BVH, flags=A.PT_FLAG_BVH_ITEMS) for p in (PARENT, NEW)}
    pairs("render_pass, Cornell 1024^2, 64 spp, pt_bvh_megakernel (BVH_ITEMS): kernel ms", {p: render_fn(p, h[p][1], 64) for p in h})
    for p in h: use(p); h[p][1].close()
if "spheres" in which:
    W, H = 1920, 1080
    kw = scenes.random_spheres(1_000_000, 7)
    mk = lambda: A.HostScene.create_arrays(**kw)
    h = {p: make(p, mk, (W, H), seed=1) for p in (PARENT, NEW)}
    pairs("config 3 (1M spheres, 1920 x 1080), 64 spp, pt_bvh_megakernel: kernel ms", {p: render_fn(p, h[p][1], 64) for p in h})
    fns = {p: ray_query_fns(p, h[p][1], W, H) for p in h}
    pairs("cast_rays, 1M spheres, 1920 x 1080 eye rays, bvh_query_kernel<false>: ms on the host's clock", {p: fns[p][0] for p in h})
    pairs("occluded, 1M spheres, 1920 x 1080 eye rays, bvh_query_kernel<true>: ms on the host's clock", {p: fns[p][1] for p in h})
    pairs("trace_paths, 1M spheres, 1920 x 1080 eye rays x 2 samples, path_query_kernel<BVH>: ms on the host's clock", {p: path_query_fn(p, h[p][1], W, H, 2) for p in h})
    for p in h: use(p); h[p][1].close()
    hp = {}
    for p in (PARENT, NEW):
        use(p); hp[p] = A.PathTracer(mk(), A.Sensor.default(W, H), seed=1, flags=A.PT_FLAG_BVH_POOL)
    pairs("config 3, 64 spp, pt_bvh_pool_kernel (lab, BVH_POOL): kernel ms", {p: render_fn(p, hp[p], 64) for p in hp})
if "lab" in which:
    W = H = 512
    for engine_name, scene, tag in (("ENGINE_LIST", A.HostScene.cornell_box, "pt_megakernel<LIST, light>"), ("ENGINE_BVH", A.HostScene.cornell_box, "pt_megakernel<BVH, light>"),
                                    ("ENGINE_REFERENCE_BVH", A.HostScene.cornell_box, "pt_megakernel<REFERENCE_BVH, light>"),
                                    ("ENGINE_AUTO", lambda: A.HostScene.create_arrays(**scenes.cornell_plus(8)), "pt_megakernel<TWO_PHASE_N, light> (33 objects)")):
        h = {p: make(p, scene, (W, H), seed=7, engine=getattr(A, engine_name)) for p in (PARENT, NEW)}
        pairs(f"lt_trace, 512^2, 4 passes, {tag}: ms on the host's clock (the whole call)", {p: lt_fn(p, h[p][1], 4) for p in h})
        pairs(f"lt_trace_photons, 512^2, 1 pass, DIFFUSE, {tag} with the vertex sink: ms on the host's clock (the whole call)", {p: photon_fn(p, h[p][1], 1) for p in h})
        for p in h: use(p); h[p][1].close()
    h = {p: make(p, A.HostScene.cornell_box, (W, H), seed=7, engine=A.ENGINE_WAVEFRONT) for p in (PARENT, NEW)}
    def wf_fn(path, pt):
        def f():
            use(path); pt.clear(); return host_ms(pt, lambda: pt.render_pass(0, 16))
        return f
    pairs("render_pass, Cornell 512^2, 16 spp, engine WAVEFRONT (wf_bounce_kernel<TWO_PHASE>): ms on the host's clock", {p: wf_fn(p, h[p][1]) for p in h})
    for p in h: use(p); h[p][1].close()
    def call_fn(path, pt, what):
        def f():
            use(path); return host_ms(pt, lambda: what(pt))
        return f
    px = np.arange(W * 64, dtype=np.uint32)
    for engine_name, flags, tag in (("ENGINE_TWO_PHASE", 0, "TWO_PHASE"), ("ENGINE_LIST", 0, "LIST"), ("ENGINE_BVH", 0, "BVH"), ("ENGINE_BVH", A.PT_FLAG_BVH_ITEMS, "BVH_ITEMS")):
        h = {p: make(p, A.HostScene.cornell_box, (W, H), seed=7, rows=(200, 264), engine=getattr(A, engine_name), flags=flags) for p in (PARENT, NEW)}
        pairs(f"render_signatures, Cornell 512 x 64 rows, 16 spp, {tag} (the render kernel's signature instantiation): ms on the host's clock", {p: call_fn(p, h[p][1], lambda pt: pt.render_signatures(0, 16)) for p in h})
        if not flags:
            pairs(f"kat_signatures, the same band, {tag} (kat_signature_kernel): ms on the host's clock", {p: call_fn(p, h[p][1], lambda pt: pt.kat_signatures(0, 16)) for p in h})
            pairs(f"kat_trace, {len(px)} paths, {tag} (kat_trace_kernel): ms on the host's clock", {p: call_fn(p, h[p][1], lambda pt: pt.kat_trace(px, np.zeros_like(px))) for p in h})
        for p in h: use(p); h[p][1].close()
    kw = scenes.random_spheres(50_000, 7)
    h = {p: make(p, lambda: A.HostScene.create_arrays(**kw), (W, H), seed=1) for p in (PARENT, NEW)}
    eye = {p: (use(p), h[p][1].kat_eye(np.arange(W * H, dtype=np.uint32), np.zeros(W * H, np.uint32)))[1] for p in h}
    def rate_fn(path, pt, e):
        def f():
            use(path); return pt.kat_traversal_rate(e[:, 0:3], e[:, 3:6], repeats=3)[2]
        return f
    pairs("kat_traversal_rate, 50 000 spheres, 512^2 eye rays, bvh_trace_rate_kernel<5, 24>: best kernel ms of 3", {p: rate_fn(p, h[p][1], eye[p]) for p in h})
    for p in h: use(p); h[p][1].close()
out = opt("--out", None)
if out:
    with open(out, "w") as f:
        f.write("\n".join(out_lines) + "\n")
sys.stdout.flush(); os._exit(0)   # several copies of the library are loaded: skip their exit-time teardown (as ab_lib.py)

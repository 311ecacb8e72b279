"""amber_hip_pt_trace_paths on the GPU (amber_amd/csrc/hip/path_query.inc): radiance along the caller's own rays.

Every comparison is on bits (uint32 / uint64 views), never within a tolerance.  The anchor is test 2: fed with the eye ray, the eye weight and the
sampler state of a rendered path, one sample gives the last measurement and the cast count of the lab's kat_trace for that path, and the whole
frame gives the bits and the ray count of render_pass.  Everything else -- known answers, chained samples, batch shapes and orders, max_depth, state
0, live updates, host against device pointers, product against lab -- is compared with calls anchored that way or with values written down here.
Frames are 24 x 16 = 384 rays (more than one workgroup, a partial last one); the batch sizes of the scheduler test sit around the wave (64), the
workgroup (256) and the claim block, with one of 4097 rays.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from amber_amd import scenes
from f64_reference import xorshift_uniform
from fuzz_scenes import scene_for_seed
from test_aov import MIXED

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
W, H, SEED, SAMPLE = 24, 16, 13, 2
N = W * H
GOLDEN = 0x9E3779B97F4A7C15


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def advanced(states, steps):
    s = np.array(states, np.uint64, copy=True)
    for _ in range(steps):
        xorshift_uniform(s)
    return s


def host_scene(amber, name):
    """(host scene, draws of its eye-ray generator): 5 for a thin lens, 2 for a pinhole"""
    if name == "cornell":
        return amber.HostScene.cornell_box(), 5
    if name == "cornell20":                                                    # 45 objects: the two-phase engine over groups of 32
        return amber.HostScene.create_arrays(**scenes.cornell_plus(20)), 5
    if name == "spheres":                                                      # AUTO picks engine BVH
        return amber.HostScene.create_arrays(**scenes.random_spheres(3000, 7)), 5
    if name == "pinhole":
        sc, _ = scene_for_seed(12)
        assert sc["n_blades"] == 0
        return amber.HostScene.create(**sc), 2
    if name == "room":                                                         # 38 triangles, a ceiling light 0.6 wide: many paths carry light
        return amber.HostScene.create_arrays(**scenes.mesh_room(0)), 5
    assert name == "mixed"                                                     # open sky, a glass sphere, a mirror sphere, four kinds of light
    return amber.HostScene.create(**MIXED), 5


def eye_inputs(amber, pt, draws, sample=SAMPLE):
    """origins, dirs, weights, states of the frame's eye paths of `sample`, as the render kernels hold them at the first cast"""
    pixel = np.arange(N, dtype=np.uint32)
    eye = pt.kat_eye(pixel, np.full(N, sample, np.uint32))
    states = advanced(amber.sampler_states(SEED, pixel, np.full(N, sample)), draws)
    return eye[:, 0:3].copy(), eye[:, 3:6].copy(), np.repeat(eye[:, 6:7], 3, axis=1), states


def tracer(amber, hs, engine="AUTO", flags=0, **kw):
    return amber.PathTracer(hs, amber.Sensor.default(W, H), seed=SEED, engine=getattr(amber, "ENGINE_" + engine), flags=flags, **kw)


# ---- 2: equal to the render kernels, path by path ---------------------------------------------------------------------------------------------
CASES = [("cornell", "LIST", 0), ("cornell", "TWO_PHASE", 0), ("cornell", "BVH", 0), ("cornell", "BVH", "PT_FLAG_BVH_ITEMS"), ("cornell", "REFERENCE_BVH", 0),
         ("cornell20", "AUTO", 0), ("spheres", "AUTO", 0), ("spheres", "AUTO", "PT_FLAG_DEVICE_BUILD"), ("pinhole", "AUTO", 0),
         ("mixed", "TWO_PHASE", 0), ("mixed", "BVH", 0), ("room", "AUTO", 0), ("room", "BVH", 0), ("room", "LIST", 0), ("room", "REFERENCE_BVH", 0)]


@pytest.mark.parametrize("name,engine,flag", CASES)
def test_equal_to_the_render_kernels_path_by_path(amber, name, engine, flag):
    assert amber.is_lab()
    hs, draws = host_scene(amber, name)
    flags = getattr(amber, flag) if flag else 0
    pt = tracer(amber, hs, engine, flags)
    o, d, w, st = eye_inputs(amber, pt, draws)
    rgb, casts, after = pt.trace_paths(o, d, w, st, n_samples=1)
    if engine == "REFERENCE_BVH":                                              # the known-answer kernels have no instantiation for this engine (its traversal
        pt.close()                                                             # stack belongs to the render kernels' grid): the frame below is its reference
    else:
        pixel, sample = np.arange(N, dtype=np.uint32), np.full(N, SAMPLE, np.uint32)
        _, kc = pt.kat_trace(pixel, sample, 1)
        rec, kc = pt.kat_trace(pixel, sample, int(kc.max()))
        pt.close()
        want = rec[np.arange(N), kc - 1, 8:11]
        lit = int((want != 0).any(axis=1).sum())
        print(f"\n{name} {engine} {flag}: casts {int(kc.min())} .. {int(kc.max())}, {lit} paths of {N} carry light")
        assert name != "room" or lit >= 10                                     # (the Cornell box's light is 0.02 wide: one sample per pixel rarely finds it)
        assert np.array_equal(casts, kc), (name, engine, int((casts != kc).sum()))
        assert np.array_equal(bits(rgb), want), (name, engine, int((bits(rgb) != want).sum()))
    assert (after != st).any() and after.dtype == np.uint64
    fresh = tracer(amber, hs, engine, flags)
    fresh.render_pass(SAMPLE, 1)
    img, rays = fresh.download()
    fresh.close()
    assert int(casts.astype(np.uint64).sum()) == rays, (name, engine, int(casts.sum()), rays)
    assert np.array_equal(bits(rgb.reshape(H, W, 3) + F32(0)), bits(img)), (name, engine)


def test_a_wavefront_handle_answers_as_auto(amber):
    """the lab engine WAVEFRONT has AUTO's closest hit"""
    hs, draws = host_scene(amber, "room")
    res = []
    for engine in ("AUTO", "WAVEFRONT"):
        pt = tracer(amber, hs, engine)
        o, d, w, st = eye_inputs(amber, pt, draws)
        res.append(pt.trace_paths(o, d, w, st, n_samples=2))
        pt.close()
    assert res[0][0].any()
    for x, y in zip(*res):
        assert x.tobytes() == y.tobytes()


# ---- 3: known answers without any kernel as reference ------------------------------------------------------------------------------------------
def cornell_light(amber, hs):
    objs, mats, _ = hs.flatten()
    rec = np.frombuffer(objs, dtype=amber.api._RECORD)
    lights = [i for i, r in enumerate(rec) if mats[int(r["material"])].kind == amber.api.MAT_DIFFUSE_LIGHT]
    r = rec[lights[0]]
    assert r["kind"] == amber.api.PRIM_TRIANGLE
    v = r["p"][:9].reshape(3, 3).astype(np.float64)
    return lights, v.mean(axis=0), r["p"][9:12].astype(np.float64), np.array(mats[int(r["material"])].rho[:], F32)


@pytest.mark.parametrize("engine", ["TWO_PHASE", "BVH", "LIST"])
def test_known_answers(amber, engine):
    hs = amber.HostScene.cornell_box()
    lights, c, n, rho = cornell_light(amber, hs)
    weights = np.array([[1, 1, 1], [0.5, 0.25, 2.5e-3], [-0.0, 0.0, 3.0], [np.inf, 1.0, -np.inf], [np.nan, 2.0, 1e-30], [7.0, -1.5, 1e30]], F32)
    k = len(weights)
    states = advanced(amber.sampler_states(99, np.arange(k), np.zeros(k)), 0)
    pt = tracer(amber, hs, engine)
    # from the front: 0.2 below the light (its normal points into the room), looking up at it
    o = np.tile(c + 0.2 * n, (k, 1)).astype(F32); d = np.tile(-n, (k, 1)).astype(F32)
    obj, _, _, _ = pt.cast_rays(o, d)
    assert set(obj.tolist()) <= set(lights)
    rgb, casts, after = pt.trace_paths(o, d, weights, states, n_samples=1)
    with np.errstate(all="ignore"):
        want = F32(0) + weights * rho
    assert np.array_equal(bits(rgb), bits(want)), (rgb, want)
    assert (casts == 1).all() and np.array_equal(after, advanced(states, 1))
    # from behind: between the light and the ceiling, looking down at its back
    o = np.tile(c - 0.005 * n, (k, 1)).astype(F32); d = np.tile(n, (k, 1)).astype(F32)
    obj, _, _, _ = pt.cast_rays(o, d)
    assert set(obj.tolist()) <= set(lights)
    rgb, casts, after = pt.trace_paths(o, d, weights, states, n_samples=1)
    finite = np.isfinite(weights).all(axis=1)                                  # (inf * 0 and NaN * 0 are NaN: as the arithmetic leaves them)
    assert finite.sum() == 4 and not bits(rgb[finite]).any() and np.isnan(rgb[~finite]).any(axis=1).all()
    assert (casts == 1).all() and np.array_equal(after, advanced(states, 1))
    # NaN in the origin or in the direction: a miss at the first cast of every sample, nothing drawn
    for col in range(6):
        od = np.concatenate([np.tile(c + 0.2 * n, (k, 1)), np.tile(-n, (k, 1))], axis=1).astype(F32)
        od[:, col] = np.nan
        rgb, casts, after = pt.trace_paths(od[:, :3], od[:, 3:], weights, states, n_samples=3)
        assert not bits(rgb).any() and (casts == 3).all() and np.array_equal(after, states), col
    pt.close()
    # rays that leave an open scene: +0, one cast, the state as it was
    pt = tracer(amber, amber.HostScene.create(**MIXED), engine)
    o = np.tile([0.0, 2.5, 0.0], (k, 1)).astype(F32); d = np.tile([0.1, 1.0, 0.2], (k, 1)).astype(F32)
    rgb, casts, after = pt.trace_paths(o, d, weights, states, n_samples=1)
    assert not bits(rgb).any() and (casts == 1).all() and np.array_equal(after, states)
    rgb, casts, after = pt.trace_paths(o, d, weights, states, n_samples=4)
    assert not bits(rgb).any() and (casts == 4).all() and np.array_equal(after, states)
    pt.close()


# ---- 4: samples chain ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,engine", [("room", "AUTO"), ("cornell", "BVH")])
def test_samples_chain(amber, name, engine):
    hs, draws = host_scene(amber, name)
    pt = tracer(amber, hs, engine)
    o, d, w, st = eye_inputs(amber, pt, draws)
    rgb5, casts5, after5 = pt.trace_paths(o, d, w, st, n_samples=5)
    total, casts, s = np.zeros((N, 3), F32), np.zeros(N, np.uint32), st
    for _ in range(5):
        r, c, s = pt.trace_paths(o, d, w, s, n_samples=1)
        total = total + r
        casts = casts + c
    assert (rgb5.any() or name != "room") and casts5.max() > 5 and np.array_equal(bits(rgb5), bits(total)) and np.array_equal(casts5, casts) and np.array_equal(after5, s)
    r2, c2, s2 = pt.trace_paths(o, d, w, st, n_samples=2)
    r3, c3, s3 = pt.trace_paths(o, d, w, s2, n_samples=3)
    assert np.array_equal(bits(rgb5), bits(r2 + r3)) and np.array_equal(casts5, c2 + c3) and np.array_equal(after5, s3)
    pt.close()


# ---- 5: the scheduler ----------------------------------------------------------------------------------------------------------------------------
def scheduler_batch(amber, pt, draws):
    """the 384 eye rays of test 2, then immediate misses and rays at the glass sphere of the mixed scene (long chains)"""
    o, d, w, st = eye_inputs(amber, pt, draws)
    rng = np.random.default_rng(3)
    m = 300
    up = np.tile([0.0, 1.8, 0.0], (m, 1)) + rng.uniform(-0.2, 0.2, (m, 3))
    up_d = np.tile([0.0, 1.0, 0.0], (m, 1)) + rng.uniform(-0.3, 0.3, (m, 3))
    g = 340
    eye = np.array([0.0, 0.2, 2.6]) + rng.uniform(-0.05, 0.05, (g, 3))
    target = np.array([0.0, -0.5, 0.8]) + rng.uniform(-0.3, 0.3, (g, 3))         # the glass sphere (radius 0.45)
    o = np.concatenate([o, up, eye]).astype(F32)
    d = np.concatenate([d, up_d, target - eye]).astype(F32)                      # (not normalised: used as given)
    w = np.concatenate([w, np.ones((m + g, 3))]).astype(F32)
    st = np.concatenate([st, amber.sampler_states(77, np.arange(m + g), np.ones(m + g))])
    return o, d, w, st


@pytest.mark.parametrize("engine", ["TWO_PHASE", "BVH"])
@pytest.mark.parametrize("n_samples", [1, 3])
def test_the_scheduler(amber, engine, n_samples):
    hs, draws = host_scene(amber, "mixed")
    pt = tracer(amber, hs, engine)
    o, d, w, st = scheduler_batch(amber, pt, draws)
    n = len(o)
    assert n == 1024
    rgb, casts, after = pt.trace_paths(o, d, w, st, n_samples=n_samples)
    print(f"\n{engine}, {n_samples} samples: casts {int(casts.min())} .. {int(casts.max())}, mean {casts.mean():.2f}")
    assert casts.min() == n_samples and casts.max() > 4 * n_samples              # items of very different length
    if n_samples == 1:                                                           # the first 384 are test 2's
        r0, c0, a0 = pt.trace_paths(o[:N], d[:N], w[:N], st[:N], n_samples=1)
        assert np.array_equal(bits(r0), bits(rgb[:N])) and np.array_equal(c0, casts[:N]) and np.array_equal(a0, after[:N])

    def same(idx, label):
        r, c, a = pt.trace_paths(o[idx], d[idx], w[idx], st[idx], n_samples=n_samples)
        assert np.array_equal(bits(r), bits(rgb[idx])) and np.array_equal(c, casts[idx]) and np.array_equal(a, after[idx]), label
    rng = np.random.default_rng(11)
    same(rng.permutation(n), "a permutation")
    same(np.argsort(casts, kind="stable")[::-1], "longest first")
    for m in (1, 63, 64, 65, 129, 255, 256, 257, 1000):                          # around the wave, the claim of 64 (and two claims and one), the workgroup
        same(np.arange(m), f"prefix {m}")
    # 4097 rays by repetition, with states of their own: every ray equals its own single-ray answer computed in another batch shape
    idx = np.arange(4097) % n
    st2 = amber.sampler_states(5, np.arange(4097), np.full(4097, 9))
    r, c, a = pt.trace_paths(o[idx], d[idx], w[idx], st2, n_samples=n_samples)
    perm = rng.permutation(4097)
    r2, c2, a2 = pt.trace_paths(o[idx][perm], d[idx][perm], w[idx][perm], st2[perm], n_samples=n_samples)
    assert np.array_equal(bits(r[perm]), bits(r2)) and np.array_equal(c[perm], c2) and np.array_equal(a[perm], a2)
    head = np.arange(70)
    r3, c3, a3 = pt.trace_paths(o[idx][head], d[idx][head], w[idx][head], st2[head], n_samples=n_samples)
    assert np.array_equal(bits(r[head]), bits(r3)) and np.array_equal(c[head], c3) and np.array_equal(a[head], a3)
    pt.close()


# ---- 6, 7: max_depth, state 0 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["TWO_PHASE", "BVH"])
def test_max_depth_of_the_call(amber, engine):
    hs, draws = host_scene(amber, "cornell")
    pt = tracer(amber, hs, engine)
    o, d, w, st = eye_inputs(amber, pt, draws)
    free = pt.trace_paths(o, d, w, st, n_samples=2)
    assert free[1].max() > 2 * 3
    capped = pt.trace_paths(o, d, w, st, n_samples=2, max_depth=3)
    assert capped[1].max() == 2 * 3 and capped[1].min() >= 2
    again = pt.trace_paths(o, d, w, st, n_samples=2, max_depth=0)                # the launch before left the handle's own value alone
    pt.close()
    for x, y in zip(free, again):
        assert x.tobytes() == y.tobytes()
    own = tracer(amber, hs, engine, max_depth=3)
    for call_depth in (0, 3):
        got = own.trace_paths(o, d, w, st, n_samples=2, max_depth=call_depth)
        for x, y in zip(capped, got):
            assert x.tobytes() == y.tobytes(), call_depth
    wider = own.trace_paths(o, d, w, st, n_samples=2, max_depth=1000)
    own.close()
    for x, y in zip(free, wider):                                              # (no path of this frame is longer than 1000)
        assert x.tobytes() == y.tobytes()


def test_state_zero(amber):
    hs, draws = host_scene(amber, "cornell")
    pt = tracer(amber, hs)
    o, d, w, _ = eye_inputs(amber, pt, draws)
    zero = pt.trace_paths(o, d, w, np.zeros(N, np.uint64), n_samples=2, max_depth=4)      # (max_depth: a build that kept the zero state would still end)
    gold = pt.trace_paths(o, d, w, np.full(N, GOLDEN, np.uint64), n_samples=2, max_depth=4)
    pt.close()
    assert zero[0].any() or zero[1].max() > 2
    for x, y in zip(zero, gold):
        assert x.tobytes() == y.tobytes()
    assert (zero[2] != 0).all()


# ---- 8: order and side effects -----------------------------------------------------------------------------------------------------------------
def test_queries_follow_updates_and_leave_the_render_alone(amber):
    from test_device_build import _objects
    from test_update_lens import _scene_kwargs
    from test_update_objects import moved
    kw_a = _scene_kwargs(amber, "A", False)
    kw_b = dict(kw_a, params=moved(kw_a, 101)["params"])
    kw_c = _scene_kwargs(amber, "B", False)                                    # the same objects under another camera: other aperture blades
    hs = {k: amber.HostScene.create_arrays(**kw) for k, kw in (("A", kw_a), ("B", kw_b), ("C", kw_c))}
    rec = {k: _objects(h) for k, h in hs.items()}
    lens = hs["A"].flatten()[2]
    blades = np.arange(lens.first_blade_object, lens.first_blade_object + lens.n_blades)
    pt = tracer(amber, hs["A"], "BVH")
    o, d, w, st = eye_inputs(amber, pt, 5)
    pt.close()
    # ... and rays at the centroids of the aperture blades of both cameras, from half a unit in front of them
    cen = np.concatenate([rec[k]["p"][blades, :9].reshape(-1, 3, 3).mean(axis=1) for k in ("A", "C")])
    nrm = np.concatenate([rec[k]["p"][blades, 9:12] for k in ("A", "C")])
    o = np.concatenate([o, cen + 0.5 * nrm, cen - 0.5 * nrm]).astype(F32); d = np.concatenate([d, -nrm, nrm]).astype(F32)
    w = np.ones((len(o), 3), F32); st = amber.sampler_states(3, np.arange(len(o)), np.zeros(len(o)))
    want = {}
    for k in hs:
        f = tracer(amber, hs[k], "BVH")
        want[k] = f.trace_paths(o, d, w, st, n_samples=2)
        f.close()
    differ = lambda x, y: any(p.tobytes() != q.tobytes() for p, q in zip(x, y))
    assert differ(want["A"], want["B"]) and differ(want["A"], want["C"])

    for mode, flags in ((amber.UPDATE_REFIT, 0), (amber.UPDATE_REBUILD, amber.PT_FLAG_DEVICE_BUILD)):   # (a rebuild needs the device's own tree)
        pt = tracer(amber, hs["A"], "BVH", flags)

        def check(key, label):
            got = pt.trace_paths(o, d, w, st, n_samples=2)
            for x, y in zip(got, want[key]):
                assert x.tobytes() == y.tobytes(), label
        pt.render_pass(0, 4)
        img, rays = pt.download()
        before = pt.kernel_time()
        check("A", "before any update")
        assert pt.kernel_time() == before                                      # no launch counted, no time added
        img2, rays2 = pt.download()
        assert rays2 == rays and np.array_equal(bits(img2), bits(img))         # the framebuffer and the ray counter as they were
        assert pt.update_flat(0, rec["B"], mode)["mode_used"] == mode; check("B", f"after update_objects {mode}")
        pt.update_flat(0, rec["A"], mode); check("A", f"back {mode}")
        pt.update_lens(hs["C"], mode); check("C", f"after update_lens {mode}")
        pt.update_lens(hs["A"], mode); check("A", f"lens back {mode}")
        pt.close()


# ---- 9: memory and errors ----------------------------------------------------------------------------------------------------------------------
def test_more_than_one_staging_trip(amber):
    """2^19 rays a trip (path_query.inc: kPathStageRays): immediate misses of the open scene around both boundaries, real paths behind them"""
    hs, draws = host_scene(amber, "mixed")
    pt = tracer(amber, hs, "TWO_PHASE")
    eo, ed, ew, est = eye_inputs(amber, pt, draws)
    want = pt.trace_paths(eo, ed, ew, est, n_samples=1)
    n = (1 << 20) + 5
    o = np.tile(np.array([0.0, 2.5, 0.0], F32), (n, 1)); d = np.tile(np.array([0.0, 1.0, 0.0], F32), (n, 1))
    w = np.ones((n, 3), F32); st = np.arange(1, n + 1, dtype=np.uint64)
    spots = {"first trip": 1000, "across the first boundary": (1 << 19) - 100, "across the second boundary": (1 << 20) - 379}
    real = np.zeros(n, bool)
    for at in spots.values():
        sl = slice(at, at + N)
        o[sl], d[sl], w[sl], st[sl], real[sl] = eo, ed, ew, est, True
    rgb, casts, after = pt.trace_paths(o, d, w, st, n_samples=1)
    pt.close()
    assert not bits(rgb[~real]).any() and (casts[~real] == 1).all() and np.array_equal(after[~real], st[~real])
    for label, at in spots.items():
        sl = slice(at, at + N)
        assert np.array_equal(bits(rgb[sl]), bits(want[0])) and np.array_equal(casts[sl], want[1]) and np.array_equal(after[sl], want[2]), label


def test_errors_leave_the_handle_as_it_was(amber):
    lib = amber.load_library()
    hs, draws = host_scene(amber, "cornell")
    for engine in ("AUTO", "BVH"):
        pt = tracer(amber, hs, engine)
        pt.render_pass(0, 4)
        want = bits(pt.download()[0]).copy()
        o, d, w, st = eye_inputs(amber, pt, draws)
        good = pt.trace_paths(o, d, w, st, n_samples=1)
        rays = np.zeros(4, amber.api._PATH_RAY); rays["dir"][:, 2] = -1; rays["origin"][:, 2] = 3; rays["weight"] = 1; rays["rng_state"] = 5
        out = np.zeros(4, amber.api._PATH_RESULT)
        fn, HOST = lib.amber_hip_pt_trace_paths, amber.RAYS_HOST
        for args, word in (((4, None, out.ctypes.data, 1, 0, HOST), "null"), ((4, rays.ctypes.data, None, 1, 0, HOST), "null"),
                           ((4, rays.ctypes.data, out.ctypes.data, 1, 0, 2), "flag"), ((4, rays.ctypes.data, out.ctypes.data, 1, 0, 0x80000001), "flag"),
                           (((1 << 31) + 1, rays.ctypes.data, out.ctypes.data, 1, 0, HOST), "2^31"), ((4, rays.ctypes.data, out.ctypes.data, 65537, 0, HOST), "65536")):
            assert fn(pt._h, *args) == -1, args                                  # AMBER_EINVAL
            msg = lib.amber_hip_last_error().decode()
            assert msg.startswith("amber_hip_pt_trace_paths: ") and word in msg, (args, msg)
        assert fn(None, 4, rays.ctypes.data, out.ctypes.data, 1, 0, HOST) == -1 and b"null handle" in lib.amber_hip_last_error()
        assert not out.view(np.uint8).any()                                    # nothing written by a refused call
        assert fn(pt._h, 0, None, None, 1, 0, 0) == 0 and fn(pt._h, 4, None, None, 0, 0, HOST) == 0      # n == 0, n_samples == 0: AMBER_OK
        rays["origin"][:, 1] = 5; rays["dir"][:, 1:3] = (1, 0)                   # above the box, going up: the largest sample count, one cast each
        assert fn(pt._h, 4, rays.ctypes.data, out.ctypes.data, 65536, 0, HOST) == 0
        assert (out["casts"] == 65536).all() and not out["rgb"].view(np.uint32).any() and (out["rng_state"] == 5).all()
        again = pt.trace_paths(o, d, w, st, n_samples=1)
        for x, y in zip(good, again):
            assert x.tobytes() == y.tobytes()
        pt.clear(); pt.render_pass(0, 4)
        assert np.array_equal(bits(pt.download()[0]), want)
        pt.close()


TORCH_CHILD = r"""
import os, sys, json
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import torch
torch.cuda.init()
import amber_amd as A
from amber_amd import scenes
from test_device_build import _objects
from test_update_objects import moved
dev = torch.device("cuda", 0)
px, sm = np.arange(384, dtype=np.uint32), np.full(384, 2, np.uint32)
st = A.sampler_states(13, px, sm)
w = np.ones((384, 3), np.float32)
def eye_rays(pt):
    eye = pt.kat_eye(px, sm)
    return eye[:, 0:3].copy(), eye[:, 3:6].copy()
same = lambda x, y: all(np.ascontiguousarray(p).tobytes() == np.ascontiguousarray(q).tobytes() for p, q in zip(x, y))
cpu = lambda ts: [t.cpu().numpy() for t in ts]
out = {{}}
kw = scenes.random_spheres(3000, 7)
kw_b = moved(kw, 101)
hs_a, hs_b = A.HostScene.create_arrays(**kw), A.HostScene.create_arrays(**kw_b)
ident = {{}}
for name, hs, engine in (("cornell", A.HostScene.cornell_box(), A.ENGINE_AUTO), ("bvh", hs_a, A.ENGINE_AUTO), ("ref_bvh", A.HostScene.cornell_box(), A.ENGINE_REFERENCE_BVH)):
    pt = A.PathTracer(hs, A.Sensor.default(24, 16), seed=13, engine=engine)
    o, d = eye_rays(pt)
    to, td, tw = (torch.from_numpy(x).to(dev) for x in (o, d, w))
    ts = torch.from_numpy(st.view(np.int64)).to(dev)
    want = pt.trace_paths(o, d, w, st, n_samples=3)
    ident[name] = []
    for stream in (None, torch.cuda.ExternalStream(pt.stream(), device=dev)):     # torch's current stream, then the handle's own
        if stream is None:
            got = pt.trace_paths(to, td, tw, ts, n_samples=3)
        else:
            with torch.cuda.stream(stream):
                got = pt.trace_paths(to, td, tw, ts, n_samples=3)
            stream.synchronize()
        g = cpu(got)
        ident[name].append(bool(same([g[0], g[1].view(np.uint32), g[2].view(np.uint64)], want)))
    # the defaults: weights 1, states sampler_state(seed, i, 0)
    g = cpu(pt.trace_paths(to, td))
    ident[name].append(bool(same([g[0], g[1].view(np.uint32), g[2].view(np.uint64)], pt.trace_paths(o, d, np.ones_like(o), A.sampler_states(13, np.arange(len(o)), np.zeros(len(o)))))))
    pt.close()
out["torch_equals_numpy"] = ident

# a query enqueued before an update answers for the old scene, one after it for the new scene (device pointers: nothing waits in between)
lib = A.load_library()
rec_b = _objects(hs_b)
order = {{}}
for mode in (A.UPDATE_REFIT, A.UPDATE_REBUILD):
    pt = A.PathTracer(hs_a, A.Sensor.default(24, 16), seed=13, flags=A.PT_FLAG_DEVICE_BUILD)
    ref = {{k: A.PathTracer(h, A.Sensor.default(24, 16), seed=13) for k, h in (("A", hs_a), ("B", hs_b))}}
    o, d = eye_rays(ref["A"])
    want = {{k: r.trace_paths(o, d, w, st, n_samples=2) for k, r in ref.items()}}
    ext = torch.cuda.ExternalStream(pt.stream(), device=dev)
    with torch.cuda.stream(ext):
        packed = torch.zeros((len(o), 16), dtype=torch.float32, device=dev)
        packed[:, 0:3], packed[:, 4:7], packed[:, 8:11] = (torch.from_numpy(x).to(dev) for x in (o, d, w))
        packed.view(torch.int64)[:, 6] = torch.from_numpy(st.view(np.int64)).to(dev)
        before, after = torch.empty((len(o), 8), dtype=torch.float32, device=dev), torch.empty((len(o), 8), dtype=torch.float32, device=dev)
        assert lib.amber_hip_pt_trace_paths(pt._h, len(o), packed.data_ptr(), before.data_ptr(), 2, 0, 0) == 0
        pt.update_flat(0, rec_b, mode)
        assert lib.amber_hip_pt_trace_paths(pt._h, len(o), packed.data_ptr(), after.data_ptr(), 2, 0, 0) == 0
    ext.synchronize()
    split = lambda x: [x[:, 0:3].contiguous().cpu().numpy(), x[:, 3].contiguous().cpu().numpy().view(np.uint32), x.view(torch.int64)[:, 2].contiguous().cpu().numpy().view(np.uint64)]
    order[str(mode)] = [bool(same(split(before), want["A"])), bool(same(split(after), want["B"])), bool(not same(want["A"], want["B"]))]
    pt.close(); [r.close() for r in ref.values()]
out["order"] = order
print("RESULT " + json.dumps(out))
"""

PRODUCT_CHILD = r"""
import os, sys, json
sys.path.insert(0, {root!r})
import numpy as np
import amber_amd as A
from amber_amd import scenes
assert A.library_path().name == "libamber_hip.so" and not A.is_lab()
for scene, hs in (("cornell", A.HostScene.cornell_box()), ("room", A.HostScene.create_arrays(**scenes.mesh_room(0)))):
    d_in = np.load(os.path.join({tmp!r}, scene + "_inputs.npz"))
    for name, engine in (("two_phase", A.ENGINE_AUTO), ("bvh", A.ENGINE_BVH), ("list", A.ENGINE_LIST), ("ref_bvh", A.ENGINE_REFERENCE_BVH)):
        pt = A.PathTracer(hs, A.Sensor.default(24, 16), seed=13, engine=engine)
        rgb, casts, after = pt.trace_paths(d_in["o"], d_in["d"], d_in["w"], d_in["st"], n_samples=3)
        np.savez(os.path.join({tmp!r}, scene + "_" + name + ".npz"), rgb=rgb, casts=casts, after=after)
        pt.close()
print("RESULT " + json.dumps(dict(ok=True)))
"""


def _child(script, env=None, timeout=600, **fmt):
    p = subprocess.run([sys.executable, "-c", script.format(root=str(ROOT), **fmt)], capture_output=True, text=True, env=env, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][7:])


def _inputs(amber, tmp_path, scene):
    hs, draws = host_scene(amber, scene)
    pt = tracer(amber, hs)
    o, d, w, st = eye_inputs(amber, pt, draws)
    pt.close()
    np.savez(tmp_path / (scene + "_inputs.npz"), o=o, d=d, w=w, st=st)
    return hs, (o, d, w, st)


def test_torch_tensors_equal_numpy_arrays_and_queries_are_stream_ordered(amber):
    assert amber.is_lab()
    res = _child(TORCH_CHILD)
    print("\n" + json.dumps(res))
    assert set(res["torch_equals_numpy"]) == {"cornell", "bvh", "ref_bvh"}
    for name, flags in res["torch_equals_numpy"].items():
        assert flags == [True, True, True], name
    for mode, (old_scene, new_scene, scenes_differ) in res["order"].items():
        assert old_scene and new_scene and scenes_differ, mode


# ---- 10: product against lab -------------------------------------------------------------------------------------------------------------------
def test_product_library_gives_the_lab_builds_bits(amber, tmp_path):
    """the Cornell box, and the room whose paths carry light"""
    assert amber.is_lab()
    mine = {scene: _inputs(amber, tmp_path, scene) for scene in ("cornell", "room")}
    _child(PRODUCT_CHILD, env=dict(os.environ, AMBER_AMD_LIB="libamber_hip.so"), tmp=str(tmp_path))
    for scene, (hs, (o, d, w, st)) in mine.items():
        for name, engine in (("two_phase", "AUTO"), ("bvh", "BVH"), ("list", "LIST"), ("ref_bvh", "REFERENCE_BVH")):
            pt = tracer(amber, hs, engine)
            rgb, casts, after = pt.trace_paths(o, d, w, st, n_samples=3)
            pt.close()
            got = np.load(tmp_path / (scene + "_" + name + ".npz"))
            assert (rgb.any() or scene != "room") and casts.max() > 3
            assert got["rgb"].tobytes() == rgb.tobytes() and got["casts"].tobytes() == casts.tobytes() and got["after"].tobytes() == after.tobytes(), (scene, name)

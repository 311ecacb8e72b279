"""amber_hip_pt_update_lens on the GPU: the camera of a live handle moved, engine BVH's tree refitted or rebuilt on the device around the new
aperture blades (amber_amd/csrc/hip/bvh_update.inc: UpdateLens).

Engine BVH's answer never depends on its tree, so the bar needs no tolerance: after the call the handle renders, light-traces and answers ray
queries with the bits of a fresh handle created on the same scene with the target camera.  The scene: 104 objects of all four primitive kinds in
[-1, 1]^3 -- past AUTO's 80-object switch to engine BVH -- some of them emitting, and a wide aperture (radius 0.4, focal length 0.02) INSIDE the
geometry, so that eye paths come back through the blades and some of the 16 x 768 light paths of lt_trace(0, 16) hit them at an angle the sensor
sees (the CPU oracle counts 127 and 72 records for cameras A and B).  Frames are 32 x 24 at 8 spp; every handle takes milliseconds.
"""
import ctypes

import numpy as np
import pytest

from bvh_parity import bits
from test_device_build import _objects

pytestmark = pytest.mark.gpu
W, H, SPP, SEED = 32, 24, 8, 21


def _transform(angle, pos):
    c, s = float(np.cos(angle)), float(np.sin(angle))
    return [c, 0, s, pos[0], 0, 1, 0, pos[1], -s, 0, c, pos[2], 0, 0, 0, 1]


# A, B: inside the geometry.  OUT: well outside the bounds of the scene as A has it (the scene diagonal and every plane word change).  NEAR: A moved
# by 1e-3 of the scene diagonal (2 sqrt(3) ~ 3.5) along every axis
CAMERAS = {"A": _transform(0.0, (0.1, 0.2, 0.5)), "B": _transform(0.6, (-0.35, 0.1, 0.3)), "OUT": _transform(0.3, (4.0, -0.5, 12.0)),
           "NEAR": _transform(0.0, (0.1 + 3.5e-3, 0.2 + 3.5e-3, 0.5 - 3.5e-3))}


def _scene_kwargs(amber, camera, pinhole):
    rng = np.random.default_rng(77)
    n = 104
    kinds = (np.arange(n) % 4).astype(np.uint32)
    params = np.zeros((n, 12), np.float32)
    c = rng.uniform(-1, 1, (n, 3))
    params[:, :3] = c
    t = kinds == 0
    params[t, 3:6] = (c + rng.normal(size=(n, 3)) * 0.25)[t]; params[t, 6:9] = (c + rng.normal(size=(n, 3)) * 0.25)[t]
    params[kinds == 1, 3] = rng.uniform(0.05, 0.2, (kinds == 1).sum())
    nrm = rng.normal(size=(n, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    for k in (2, 3):
        params[kinds == k, 3:6] = nrm[kinds == k]
        params[kinds == k, 6] = rng.uniform(0.05, 0.2, (kinds == k).sum())
    params[kinds == 3, 7] = rng.uniform(0.1, 0.4, (kinds == 3).sum())
    materials = [(amber.api.MAT_DIFFUSE_LIGHT, (6.0, 5.0, 4.0), 0.0), (amber.api.MAT_LAMBERTIAN, (0.7, 0.7, 0.7), 0.0), (amber.api.MAT_SPECULAR, (0.9, 0.9, 0.9), 0.0),
                 (amber.api.MAT_REFRACTION, (1.0, 1.0, 1.0), 1.5), (amber.api.MAT_PHONG, (0.8, 0.8, 0.8), 30.0)]
    material_index = rng.integers(0, len(materials), n).astype(np.uint32)
    material_index[:len(materials)] = np.arange(len(materials))              # every material in use, in the same order of first appearance for every camera
    return dict(kinds=kinds, material_index=material_index, params=params, materials=materials, transform=CAMERAS[camera], focal_length=0.02,
                focus_distance=1.5, radius=0.4, n_blades=0 if pinhole else 6)


class Views:
    """One scene under every camera, with a thin lens or a pinhole: the host scenes, their flattened records and lenses, and what a FRESH handle
    (engine BVH, the host's tree) gives for each -- image bits, ray count, the record list of lt_trace(0, 16) -- computed once and left unchanged."""
    def __init__(self, amber, pinhole):
        self.amber, self.pinhole = amber, pinhole
        self.hs = {k: amber.HostScene.create_arrays(**_scene_kwargs(amber, k, pinhole)) for k in CAMERAS}
        self.rec = {k: _objects(h) for k, h in self.hs.items()}
        self.lens = {k: h.flatten()[2] for k, h in self.hs.items()}
        L = self.lens["A"]
        self.first, self.n_blades = int(L.first_blade_object), int(L.n_blades)
        self.blade_ids = np.arange(self.first, self.first + self.n_blades)
        rest = np.delete(np.arange(len(self.rec["A"])), self.blade_ids)
        for k in CAMERAS:                                                    # the cameras differ in the lens values and the blades' geometry, in nothing else
            assert (int(self.lens[k].first_blade_object), int(self.lens[k].n_blades), int(self.lens[k].kind)) == (self.first, self.n_blades, int(L.kind))
            assert self.rec[k][rest].tobytes() == self.rec["A"][rest].tobytes()
            assert np.array_equal(self.rec[k]["material"], self.rec["A"]["material"]) and (self.rec[k]["kind"][self.blade_ids] == 0).all()
            assert k == "A" or self.rec[k][self.blade_ids].tobytes() != self.rec["A"][self.blade_ids].tobytes()
        assert len(self.rec["A"]) > 100 and set(self.rec["A"]["kind"]) == {0, 1, 2, 3}
        self._fresh = {}

    def blades(self, key):
        return self.rec[key][self.blade_ids].copy()

    def tracer(self, key, engine=None, device=False):
        a = self.amber
        return a.PathTracer(self.hs[key], a.Sensor.default(W, H), seed=SEED, engine=a.ENGINE_BVH if engine is None else engine,
                            flags=a.PT_FLAG_DEVICE_BUILD if device else 0)

    def look(self, pt):
        """(image bits, rays, lt records as bytes, lt rays) of the handle as it stands; the framebuffer is cleared first"""
        pt.clear()
        pt.render_pass(0, SPP)
        img, rays = pt.download()
        splats, lt_rays = pt.lt_trace(0, 16)
        return bits(img).copy(), rays, splats.tobytes(), lt_rays

    def fresh(self, key):
        if key not in self._fresh:
            pt = self.tracer(key)
            self._fresh[key] = self.look(pt)
            pt.close()
        return self._fresh[key]


_views = {}


def views(amber, pinhole=False):
    if pinhole not in _views:
        _views[pinhole] = Views(amber, pinhole)
    return _views[pinhole]


def same(got, want, label):
    assert got[1] == want[1], (label, "rays", got[1], want[1])
    assert np.array_equal(got[0], want[0]), (label, "pixels that differ", int((got[0] != want[0]).sum()))
    assert got[3] == want[3] and got[2] == want[2], (label, "lt_trace", got[3], want[3])


def test_the_views_are_worth_comparing(amber):
    """paths come back through the aperture and light paths reach the sensor: every camera inside the scene sees something, and no two views are the same"""
    for pinhole in (False, True):
        V = views(amber, pinhole)
        got = {k: V.fresh(k) for k in CAMERAS}
        for k in ("A", "B", "NEAR"):
            assert got[k][0].any() and got[k][1] > W * H * SPP, k
        assert got["A"][0].tobytes() != got["B"][0].tobytes() != got["OUT"][0].tobytes()
        assert got["A"][3] > 0                                               # light paths are traced under either lens; they reach the sensor only by
        if not pinhole:                                                      # hitting a blade (algorithm_lt.cc:142-148), which a pinhole's degenerate one never is
            assert got["A"][3] != got["B"][3] and got["A"][2] != got["B"][2] and len(got["A"][2]) >= 32 * 50 and len(got["B"][2]) >= 32 * 50


# ---- 1: updated == fresh, bit for bit: image, ray count, light-tracing records -------------------------------------------------------------------
@pytest.mark.parametrize("pinhole", [False, True], ids=["thin", "pinhole"])
@pytest.mark.parametrize("start", ["host_tree", "device_tree"])
@pytest.mark.parametrize("mode", ["refit", "rebuild"])
@pytest.mark.parametrize("engine", ["ENGINE_BVH", "ENGINE_AUTO"])
def test_a_handle_with_a_new_lens_equals_a_fresh_one(amber, engine, mode, start, pinhole):
    V, m = views(amber, pinhole), (amber.UPDATE_REFIT if mode == "refit" else amber.UPDATE_REBUILD)
    pt = V.tracer("A", engine=getattr(amber, engine), device=start == "device_tree")
    same(V.look(pt), V.fresh("A"), "before")                                # warm state: buffers sized, passes behind the handle
    info = pt.update_lens(V.hs["B"], m)
    print(f"\n{engine}, {mode}, {start}, {'pinhole' if pinhole else 'thin lens'}: {info}")
    assert info["mode_used"] == m and info["fallback_reason"] == 0 and info["update_ms"] > 0, info
    same(V.look(pt), V.fresh("B"), "after update_lens(scene B)")
    info = pt.update_lens((V.lens["A"], V.blades("A")), m)                   # the explicit pair
    assert info["mode_used"] == m
    same(V.look(pt), V.fresh("A"), "after update_lens((lens A, blades A))")
    pt.close()


# ---- 2: far and near ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["refit", "rebuild"])
@pytest.mark.parametrize("target", ["OUT", "NEAR"])
def test_a_camera_moved_outside_the_bounds_and_one_moved_by_a_thousandth_of_the_diagonal(amber, target, mode):
    V, m = views(amber), (amber.UPDATE_REFIT if mode == "refit" else amber.UPDATE_REBUILD)
    if target == "OUT":                                                     # really outside: farther from the centre than any object of A's scene reaches
        assert np.abs(np.array(V.lens["OUT"].origin[:])).max() > 2.0 * np.abs(V.rec["A"]["p"][:, :9]).max()
    pt = V.tracer("A")
    built = pt.build_info()
    same(V.look(pt), V.fresh("A"), "before")
    info = pt.update_lens(V.hs[target], m)
    assert info["mode_used"] == m and np.isfinite(info["area_after"]) and np.isfinite(info["area_before"]) and info["area_after"] > 0, info
    same(V.look(pt), V.fresh(target), target)
    bi = pt.build_info()
    if m == amber.UPDATE_REBUILD:
        assert bi["where"] == amber.BUILD_DEVICE and (bi["n_nodes"], bi["n_leaves"], bi["depth"]) == (info["n_nodes"], info["n_nodes"] + 1, info["depth"]), (bi, info)
    else:
        assert bi == built and (info["n_nodes"], info["depth"]) == (built["n_nodes"], built["depth"])
    info = pt.update_lens(V.hs["A"], m)                                     # and home again
    assert np.isfinite(info["area_after"])
    same(V.look(pt), V.fresh("A"), "back to A")
    pt.close()


# ---- 3: ray queries ------------------------------------------------------------------------------------------------------------------------------------
def _aperture_rays(V, key):
    """two rays per blade of camera `key`, from 1e-3 in front of and behind its centroid towards it, t_max 1e-2: only the blade is that close"""
    p = V.blades(key)["p"]
    centroid = (p[:, 0:3] + p[:, 3:6] + p[:, 6:9]) / np.float32(3)
    n = p[:, 9:12]
    o = np.concatenate([centroid + np.float32(1e-3) * n, centroid - np.float32(1e-3) * n]).astype(np.float32)
    d = np.concatenate([-n, n]).astype(np.float32)
    return o, d, np.tile(V.blade_ids, 2)


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_ray_queries_find_the_new_blades_and_not_the_old_ones(amber, mode):
    V, m = views(amber), (amber.UPDATE_REFIT if mode == "refit" else amber.UPDATE_REBUILD)
    o_a, d_a, ids = _aperture_rays(V, "A")
    o_b, d_b, _ = _aperture_rays(V, "B")
    o, d = np.concatenate([o_a, o_b]), np.concatenate([d_a, d_b])
    old, new = slice(0, len(o_a)), slice(len(o_a), len(o))
    want = {}
    for key in "AB":
        pt = V.tracer(key)
        want[key] = (pt.cast_rays(o, d, 1e-2), pt.occluded(o, d, 1e-2))
        pt.close()
    hit_a, hit_b = want["A"][0][0], want["B"][0][0]
    assert np.array_equal(hit_a[old], ids) and np.array_equal(hit_b[new], ids)        # each camera's own blades, by scene index
    assert not np.isin(hit_a[new], V.blade_ids).any() and not np.isin(hit_b[old], V.blade_ids).any()

    pt = V.tracer("A", device=mode == "rebuild")
    # a query enqueued BEFORE the update (device pointers: asynchronous on the handle's stream) answers for the old lens
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    packed, n, _ = pt._pack_rays(o, d, 1e-2)
    d_rays, d_hits = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(d_rays), packed.nbytes) == 0 and hip.hipMalloc(ctypes.byref(d_hits), 32 * n) == 0
    try:
        assert hip.hipMemcpy(d_rays, packed.ctypes.data, packed.nbytes, 1) == 0          # hipMemcpyHostToDevice
        assert amber.load_library().amber_hip_pt_cast_rays(pt._h, n, d_rays, d_hits, 0) == 0
        info = pt.update_lens(V.hs["B"], m)
        assert info["mode_used"] == m
        before = np.zeros(n, np.dtype([("t", np.float32), ("object", np.int32), ("pos", np.float32, (3,)), ("normal", np.float32, (3,))]))   # AmberRayHit
        assert hip.hipMemcpy(before.ctypes.data, d_hits, 32 * n, 2) == 0                 # hipMemcpyDeviceToHost
    finally:
        hip.hipFree(d_rays); hip.hipFree(d_hits)
    assert np.array_equal(before["object"], hit_a) and np.array_equal(bits(before["t"]), bits(want["A"][0][1]))
    got = (pt.cast_rays(o, d, 1e-2), pt.occluded(o, d, 1e-2))
    pt.close()
    for g, w in zip(got[0], want["B"][0]):                                  # object, t, pos, normal: the fresh handle's bytes
        assert g.tobytes() == w.tobytes()
    assert np.array_equal(got[1], want["B"][1])
    assert np.array_equal(got[0][0][new], ids) and got[1][new].all()        # the new blades' scene indices
    assert not np.isin(got[0][0][old], V.blade_ids).any()                   # nothing of the aperture is left at the old position


# ---- 4: object updates around a lens update ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_object_updates_before_and_after_a_lens_update(amber, mode):
    V, m = views(amber), (amber.UPDATE_REFIT if mode == "refit" else amber.UPDATE_REBUILD)
    moved = V.rec["A"].copy()                                               # every object but the blades and the emitters (a moved emitter makes the lights
    shift = np.array([0.01, -0.02, 0.015], np.float32)                      # table stale: update_objects' rule) shifted a little; A's blades stay in the range
    emits = np.array([m.kind == amber.api.MAT_DIFFUSE_LIGHT for m in V.hs["A"].flatten()[1]])[moved["material"]]
    rest = ~np.isin(np.arange(len(moved)), V.blade_ids) & ~emits
    assert 20 < rest.sum() < len(moved) - V.n_blades
    tri = moved["kind"] == 0
    for v in range(3):
        sel = rest & (tri | (v == 0))
        moved["p"][sel, 3 * v:3 * v + 3] += shift
    pt = V.tracer("A")
    pt.update_flat(0, moved, m)
    pt.update_lens(V.hs["B"], m)
    after_lens = V.look(pt)
    with pytest.raises(amber.AmberError, match=f"object {V.first} is an aperture blade"):
        pt.update_flat(0, V.rec["A"], m)                                    # the whole scene with the OLD blades: refused, and nothing has changed
    same(V.look(pt), after_lens, "after the refused update")
    pt.update_flat(0, V.rec["B"], m)                                        # with the new blades: accepted; the objects are back where scene B has them
    same(V.look(pt), V.fresh("B"), "objects -> lens -> objects")
    pt.update_flat(V.first, V.blades("B"), m)                               # the blades alone
    same(V.look(pt), V.fresh("B"), "blades alone")
    pt.close()


# ---- 5: refusals leave the handle alone -----------------------------------------------------------------------------------------------------------------
def _lens_copy(lens, **changes):
    out = type(lens).from_buffer_copy(lens)
    for k, v in changes.items():
        setattr(out, k, v)
    return out


def test_refusals_leave_the_handle_as_it_was(amber):
    V = views(amber)
    L, B = V.lens["B"], V.blades("B")
    pt = V.tracer("A")
    want = V.look(pt)
    more = np.concatenate([B, B[:1]])

    def bad(pair, match, mode=amber.UPDATE_REFIT):
        with pytest.raises(amber.AmberError, match=match):
            pt.update_lens(pair, mode)
        same(V.look(pt), want, match)

    for mode in (amber.UPDATE_REFIT, amber.UPDATE_REBUILD):
        bad((_lens_copy(L, n_blades=V.n_blades + 1), more), "amber error -1: .*differ from the resident lens", mode)
        bad((_lens_copy(L, n_blades=V.n_blades - 1), B), "amber error -1: .*differ from the resident lens", mode)
        bad((_lens_copy(L, kind=1 - int(L.kind)), B), "amber error -1: .*differ from the resident lens", mode)
        bad((_lens_copy(L, first_blade_object=V.first + 1), B), "amber error -1: .*differ from the resident lens", mode)
        bad((None, B), "amber error -1: .*null lens or blades", mode)
        bad((L, None), "amber error -1: .*null lens or blades", mode)
        wrong = B.copy(); wrong["kind"][1] = amber.api.PRIM_SPHERE
        bad((L, wrong), "amber error -1: .*blade 1 is not a triangle", mode)
        wrong = B.copy(); wrong["material"][2] += 1
        bad((L, wrong), "amber error -1: .*blade 2 is not a triangle of the resident blade's material", mode)
    bad((L, B), "amber error -1: .*unknown mode", mode=7)
    pt.close()
    for engine in (amber.ENGINE_TWO_PHASE, amber.ENGINE_LIST, amber.ENGINE_REFERENCE_BVH):
        pt = V.tracer("A", engine=engine)
        before = V.look(pt)
        for mode in (amber.UPDATE_REFIT, amber.UPDATE_REBUILD):
            with pytest.raises(amber.AmberError, match="amber error -1: .*re-create"):
                pt.update_lens(V.hs["B"], mode)
        same(V.look(pt), before, f"engine {engine}")
        pt.close()


# ---- 6: there and back ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_two_lens_updates_in_a_row_come_back_to_the_first_image(amber, mode):
    V, m = views(amber), (amber.UPDATE_REFIT if mode == "refit" else amber.UPDATE_REBUILD)
    pt = V.tracer("A", device=mode == "rebuild")
    first = V.look(pt)
    pt.update_lens(V.hs["B"], m)
    pt.update_lens(V.hs["A"], m)                                            # (no pass between the two: the second one fills the other buffer)
    same(V.look(pt), first, "A -> B -> A")
    pt.update_lens(V.hs["OUT"], m)
    same(V.look(pt), V.fresh("OUT"), "A -> B -> A -> OUT")
    pt.close()


def test_a_pass_enqueued_before_the_lens_update_renders_the_old_view(amber):
    V = views(amber)
    parts = []
    for key, first in (("A", 0), ("B", SPP)):
        pt = V.tracer(key)
        pt.render_pass(first, SPP)
        parts.append(pt.download())
        pt.close()
    pt = V.tracer("A")
    pt.render_pass(0, SPP)
    pt.update_lens(V.hs["B"])                                               # mode defaults to UPDATE_REFIT; the framebuffer is not cleared
    pt.render_pass(SPP, SPP)
    img, rays = pt.download()
    pt.close()
    assert rays == parts[0][1] + parts[1][1]
    assert np.array_equal(bits(img), bits((parts[0][0] + parts[1][0]).astype(np.float32)))

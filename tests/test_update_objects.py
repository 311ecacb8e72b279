"""amber_hip_pt_update_objects on the GPU: new geometry for a live handle, engine BVH's tree refitted or rebuilt on the device
(amber_amd/csrc/hip/bvh_update.inc).

Engine BVH's answer never depends on its tree, so the bar needs no tolerance: an updated handle renders the bits a fresh handle created on the
new scene renders.  Scene B is scene A with every object translated rigidly by a seeded random vector no longer than half its own largest box
side and 1 % of the scene extent, sphere radii scaled by 0.8 ... 1.25, aperture blades untouched.  Refit tests keep the motion bounded by the
objects' own size on purpose: a refit after scrambling the objects is a valid tree whose every box spans the scene, and rendering through it
could hold a shared GPU for minutes.  Large motion (a seeded permutation of the centres) is tested with REBUILD only.
"""
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest

import oracle_binding as O
from amber_amd import scenes
from amber_amd import workloads as WL
from bvh_parity import bits
from test_device_build import _decode, _mixed_scene, _nan_scene, _objects, _random_rays, validate_tree

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
MAT_DIFFUSE_LIGHT = 4

# frame, seed, rows, spp: those of test_host_and_device_trees_render_the_same_bits (the mixed scene has no entry there)
FRAMES = {"spheres": (1024, 1024, 7, (500, 516), 16), "room": (1024, 1024, 7, (640, 656), 16), "terrain": (1920, 1080, 3, (800, 816), 8),
          "mixed": (512, 512, 5, (240, 256), 16)}


def _scene_kwargs(which):
    if which == "spheres":
        return scenes.random_spheres(50_000, 7)
    if which == "room":
        return WL.room_mesh(3).arrays()
    if which == "terrain":
        return WL.terrain_mesh(16, 56).arrays()
    return _mixed_scene()


def _box_sides(kinds, p):
    tri = p[:, :9].reshape(-1, 3, 3)
    side = np.where(kinds == 0, (tri.max(1) - tri.min(1)).max(1), 0.0)
    side = np.where(kinds == 1, 2.0 * np.abs(p[:, 3]), side)
    side = np.where(kinds == 2, 2.0 * np.abs(p[:, 6]), side)
    return np.where(kinds == 3, 2.0 * np.maximum(np.abs(p[:, 6]), np.abs(p[:, 7])), side)


def moved(kw, seed, keep_emitters=False):
    """kw with every object translated by a vector no longer than half its largest box side and 1 % of the scene extent, sphere radii scaled"""
    rng = np.random.default_rng(seed)
    kinds, p = np.asarray(kw["kinds"]), np.array(kw["params"], np.float32, copy=True)
    full = np.zeros((len(p), 12), np.float32); full[:, :p.shape[1]] = p
    p, n = full, len(full)
    extent = float((np.nanmax(p[:, :3], 0) - np.nanmin(p[:, :3], 0)).max())
    limit = np.minimum(0.5 * _box_sides(kinds, p), 0.01 * extent)
    direction = rng.normal(size=(n, 3)); direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    shift = direction * (rng.uniform(0, 1, n) * limit)[:, None]
    scale = rng.uniform(0.8, 1.25, n)
    if keep_emitters:
        emit = np.array([kw["materials"][m][0] == MAT_DIFFUSE_LIGHT for m in np.asarray(kw["material_index"])])
        shift[emit] = 0.0; scale[emit] = 1.0
    shift = shift.astype(np.float32)
    tri = kinds == 0
    for v in range(3):
        p[:, 3 * v:3 * v + 3] = np.where((tri | (v == 0))[:, None], p[:, 3 * v:3 * v + 3] + shift, p[:, 3 * v:3 * v + 3])
    p[:, 3] = np.where(kinds == 1, (p[:, 3] * scale).astype(np.float32), p[:, 3])
    return dict(kw, params=p)


def permuted(kw, seed):
    """large motion: the centres of the spheres change places"""
    rng = np.random.default_rng(seed)
    p = np.array(kw["params"], np.float32, copy=True)
    p[:, :3] = p[rng.permutation(len(p)), :3]
    return dict(kw, params=p)


class Scenes:
    """A, B, C of one scene, their flattened records, and what a fresh handle renders of each (host tree), computed once"""
    def __init__(self, amber, which):
        self.amber, self.which = amber, which
        a = _scene_kwargs(which)
        self.kw = {"A": a, "B": moved(a, 101, keep_emitters=which == "room"), "C": moved(a, 202)}
        self.hs = {k: amber.HostScene.create_arrays(**v) for k, v in self.kw.items()}
        self.rec = {k: _objects(h) for k, h in self.hs.items()}
        lens = self.hs["A"].flatten()[2]                                    # where the aperture blades are: from the flattened lens
        self.first_blade, self.n_blades = int(lens.first_blade_object), int(lens.n_blades)
        self.blades = np.arange(self.first_blade, self.first_blade + self.n_blades)
        self.user = np.delete(np.arange(len(self.rec["A"])), self.blades)   # scene index of the caller's object j (create_arrays keeps their order)
        assert len(self.user) == len(a["kinds"]) and self.n_blades > 0
        for k in "BC":                                                      # an update keeps kinds and materials; the blades are where they were
            assert np.array_equal(self.rec[k]["kind"], self.rec["A"]["kind"]) and np.array_equal(self.rec[k]["material"], self.rec["A"]["material"])
        self.W, self.H, self.seed, self.rows, self.spp = FRAMES[which]
        self._fresh, self._dump = {}, {}

    def tracer(self, key, device=False, rows=None, **kw):
        a = self.amber
        return a.PathTracer(self.hs[key], a.Sensor.default(self.W, self.H), seed=self.seed, rows=rows or self.rows, flags=a.PT_FLAG_DEVICE_BUILD if device else 0, **kw)

    def band(self, pt):
        pt.render_pass(0, self.spp)
        img, rays = pt.download()
        return bits(img).copy(), rays

    def fresh(self, key):
        """(image bits, rays, signatures of four rows) of a fresh handle with the host's tree"""
        if key not in self._fresh:
            pt = self.tracer(key)
            img, rays = self.band(pt)
            pt.close()
            pt = self.tracer(key, rows=(self.rows[0], self.rows[0] + 4))
            sig = pt.render_signatures(0, 8)
            pt.close()
            self._fresh[key] = (img, rays, sig)
        return self._fresh[key]

    def device_dump(self, key):
        if key not in self._dump:
            pt = self.tracer(key, device=True)
            self._dump[key] = (pt.bvh_dump(), pt.build_info())
            pt.close()
        return self._dump[key]


_cache = {}


@pytest.fixture
def sc(amber, request):
    which = request.param
    if which not in _cache:
        _cache.clear()                                                      # one scene's host copies at a time
        _cache[which] = Scenes(amber, which)
    return _cache[which]


def _same_dump(a, b, keys=("nodes", "prims", "gmin", "step", "reach")):
    return all(a[k].tobytes() == b[k].tobytes() for k in keys) and a["root"] == b["root"] and a["depth"] == b["depth"]


def _check_tree_after(amber, S, pt, key, mode, before, info):
    dump = pt.bvh_dump()
    st = validate_tree(dump, S.rec[key], f"{S.which} -> {key}, mode {mode}")
    assert info["n_nodes"] == st["nodes"] == len(dump["nodes"]) and info["depth"] == st["depth"]
    if info["mode_used"] == amber.UPDATE_REFIT:
        assert dump["nodes"][:, 6:8].tobytes() == before["nodes"][:, 6:8].tobytes() and dump["prims"].tobytes() == before["prims"].tobytes()
        assert dump["depth"] == before["depth"] and dump["root"] == before["root"]
    else:
        fresh_dump, fresh_info = S.device_dump(key)
        assert _same_dump(dump, fresh_dump), "a rebuilt tree is a function of the scene alone"
        bi = pt.build_info()
        assert bi["where"] == amber.BUILD_DEVICE and (bi["n_nodes"], bi["n_leaves"], bi["depth"]) == (info["n_nodes"], info["n_nodes"] + 1, info["depth"])
        assert (bi["n_nodes"], bi["depth"]) == (fresh_info["n_nodes"], fresh_info["depth"])
    return dump


# ---- 1 and 3: updated == fresh, bit for bit; the tree is valid by the host builder's rules -------------------------------------------------
@pytest.mark.parametrize("mode", ["refit", "rebuild"])
@pytest.mark.parametrize("start", ["host_tree", "device_tree"])
@pytest.mark.parametrize("sc", ["spheres", "room", "terrain", "mixed"], indirect=True)
def test_an_updated_handle_renders_the_bits_of_a_fresh_one(amber, sc, start, mode):
    S, m = sc, (amber.UPDATE_REFIT if mode == "refit" else amber.UPDATE_REBUILD)
    pt = S.tracer("A", device=start == "device_tree")
    first_a = S.band(pt)                                                    # warm state: buffers sized, a pass behind the handle
    assert first_a[1] == S.fresh("A")[1] and np.array_equal(first_a[0], S.fresh("A")[0])
    info_before = pt.build_info()
    before = pt.bvh_dump()
    for key in ("B", "C", "A"):
        info = pt.update_flat(0, S.rec[key], m)
        assert info["mode_used"] == m and info["fallback_reason"] == 0 and info["update_ms"] > 0, info
        assert info["area_before"] > 0 and info["area_after"] > 0
        print(f"\n{S.which}, {start}, {mode} -> {key}: {info}")
        pt.clear()
        img, rays = S.band(pt)
        want = S.fresh(key)
        assert rays == want[1], (key, rays, want[1])
        assert np.array_equal(img, want[0]), (key, int((img != want[0]).sum()))
        before = _check_tree_after(amber, S, pt, key, m, before, info)
        if m == amber.UPDATE_REFIT:
            assert pt.build_info() == info_before                          # a refit leaves build_info alone
    assert np.array_equal(img, first_a[0]) and rays == first_a[1]           # B -> C -> A: the very first render again
    pt.close()
    pt = S.tracer("A", device=start == "device_tree", rows=(S.rows[0], S.rows[0] + 4))
    pt.update_flat(0, S.rec["B"], m)
    assert np.array_equal(pt.render_signatures(0, 8), S.fresh("B")[2])
    pt.close()
    if S.which == "room":                                                   # B moves no emitting object: light tracing still answers, as a fresh handle does
        splats = []
        for updated in (False, True):
            pt = amber.PathTracer(S.hs["A" if updated else "B"], amber.Sensor.default(64, 48), seed=3, flags=amber.PT_FLAG_DEVICE_BUILD if start == "device_tree" else 0)
            if updated:
                pt.update_flat(0, S.rec["B"], m)
            splats.append(pt.lt_trace(0, 16))
            pt.close()
        assert splats[0][1] == splats[1][1] > 0 and splats[0][0].tobytes() == splats[1][0].tobytes()


@pytest.mark.parametrize("sc", ["spheres", "terrain"], indirect=True)
def test_a_refit_with_the_same_objects_leaves_a_device_built_tree_as_it_was(amber, sc):
    S = sc
    pt = S.tracer("A", device=True)
    before = pt.bvh_dump()
    info = pt.update_flat(0, S.rec["A"], amber.UPDATE_REFIT)
    assert _same_dump(pt.bvh_dump(), before), info
    assert abs(info["area_after"] / info["area_before"] - 1) < 1e-5
    pt.close()


# ---- 2: partial ranges -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc", ["spheres", "room"], indirect=True)
def test_partial_ranges(amber, sc):
    S = sc
    n = len(S.rec["A"])
    for lo, hi in ((n // 3, n // 3 + n // 100), (n - 5, n)):
        rec = S.rec["A"].copy()
        rec[lo:hi] = S.rec["C"][lo:hi]
        kw = dict(S.kw["A"])
        p = np.zeros((len(S.user), 12), np.float32); p[:] = rec["p"][S.user]
        hs = amber.HostScene.create_arrays(**dict(kw, params=p))
        assert _objects(hs).tobytes() == rec.tobytes()                      # the fresh handle's scene is the one the update makes
        pt = amber.PathTracer(hs, amber.Sensor.default(S.W, S.H), seed=S.seed, rows=S.rows)
        want = S.band(pt)
        pt.close()
        for mode in (amber.UPDATE_REFIT, amber.UPDATE_REBUILD):
            pt = S.tracer("A", device=mode == amber.UPDATE_REBUILD)
            S.band(pt)
            pt.update_flat(lo, rec[lo:hi], mode)
            pt.clear()
            img, rays = S.band(pt)
            validate_tree(pt.bvh_dump(), rec, "partial range")
            pt.close()
            assert rays == want[1] and np.array_equal(img, want[0]), (lo, hi, mode)


# ---- the documented Python call: arrays as HostScene.create_arrays takes them ---------------------------------------------------------------------
@pytest.mark.parametrize("sc", ["spheres", "room", "mixed"], indirect=True)
def test_update_objects_takes_the_arrays_create_arrays_takes(amber, sc):
    """PathTracer.update_objects(first, kinds, material_index, params, mode) with the caller's own arrays -- user material indices, (n, 9) triangle
    parameters without normals, disk / cylinder axes that are not unit vectors -- gives the bits of a fresh handle: all the caller's objects, then a
    partial range back to A."""
    S = sc
    kwa, kwb = S.kw["A"], S.kw["B"]
    assert np.array_equal(S.user, np.arange(S.user[0], S.user[0] + len(S.user)))   # the caller's objects are one run of scene indices
    cols = 9 if S.which == "room" else 12
    for mode in (amber.UPDATE_REFIT, amber.UPDATE_REBUILD):
        pt = S.tracer("A", device=mode == amber.UPDATE_REBUILD)
        S.band(pt)
        info = pt.update_objects(int(S.user[0]), kwb["kinds"], kwb["material_index"], np.asarray(kwb["params"])[:, :cols], mode)
        assert info["mode_used"] == mode
        pt.clear()
        img, rays = S.band(pt)
        validate_tree(pt.bvh_dump(), S.rec["B"], "update_objects")
        assert rays == S.fresh("B")[1] and np.array_equal(img, S.fresh("B")[0]), mode
        m = len(S.user)
        lo, hi = m // 3, m // 3 + m // 2                                    # these go back to A; the rest stay B's
        pt.update_objects(int(S.user[lo]), kwa["kinds"][lo:hi], kwa["material_index"][lo:hi], np.asarray(kwa["params"])[lo:hi, :cols], mode)
        rec = S.rec["B"].copy(); rec[S.user[lo:hi]] = S.rec["A"][S.user[lo:hi]]
        pt.clear()
        img, rays = S.band(pt)
        pt.close()
        p = np.zeros((m, 12), np.float32); p[:] = rec["p"][S.user]
        hs = amber.HostScene.create_arrays(**dict(kwa, params=p))
        assert _objects(hs).tobytes() == rec.tobytes()
        ref = amber.PathTracer(hs, amber.Sensor.default(S.W, S.H), seed=S.seed, rows=S.rows)
        want = S.band(ref)
        ref.close()
        assert rays == want[1] and np.array_equal(img, want[0]), mode
    pt = S.tracer("A")
    with pytest.raises(amber.AmberError, match="kind differs"):
        pt.update_objects(int(S.user[0]), (np.asarray(kwb["kinds"]) + 1) % 4, kwb["material_index"], kwb["params"])
    shuffled = np.asarray(kwb["material_index"]).copy(); shuffled[: len(shuffled) // 2] = shuffled[0]
    with pytest.raises(amber.AmberError, match="material"):
        pt.update_objects(int(S.user[0]), kwb["kinds"], shuffled, kwb["params"])
    pt.close()


# ---- large motion: REBUILD only ------------------------------------------------------------------------------------------------------------------
def test_a_rebuild_after_the_centres_changed_places(amber):
    kw_a = scenes.random_spheres(50_000, 7)
    kw_b = permuted(kw_a, 9)
    hs_a, hs_b = amber.HostScene.create_arrays(**kw_a), amber.HostScene.create_arrays(**kw_b)
    W, H, seed, rows, spp = FRAMES["spheres"]
    pt = amber.PathTracer(hs_b, amber.Sensor.default(W, H), seed=seed, rows=rows)
    pt.render_pass(0, spp); want, want_rays = pt.download(); pt.close()
    pt = amber.PathTracer(hs_b, amber.Sensor.default(W, H), seed=seed, rows=rows, flags=amber.PT_FLAG_DEVICE_BUILD)
    fresh_dump = pt.bvh_dump(); pt.close()
    pt = amber.PathTracer(hs_a, amber.Sensor.default(W, H), seed=seed, rows=rows)
    info = pt.update_flat(0, _objects(hs_b), amber.UPDATE_REBUILD)
    assert info["mode_used"] == amber.UPDATE_REBUILD
    pt.render_pass(0, spp); img, rays = pt.download()
    assert _same_dump(pt.bvh_dump(), fresh_dump)
    pt.close()
    assert rays == want_rays and np.array_equal(bits(img), bits(want))


# ---- 4: closest hits against the oracle, through a refitted handle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sc", ["spheres", "room", "terrain"], indirect=True)
def test_closest_hits_of_a_refitted_tree_equal_the_list_oracle(amber, sc):
    S = sc
    W, H, seed, rows = {"spheres": (1024, 1024, 7, (500, 503)), "room": (1024, 1024, 7, (650, 653)), "terrain": (1920, 1080, 3, (810, 812))}[S.which]
    osc = O.Scene.create_arrays(**S.kw["B"], accel=O.ACCEL_BVH_CONS)
    o1, d1 = osc.collect_rays(W, H, seed, 0, 2, rows, 40_000)
    o2, d2 = _random_rays(S.rec["B"], 100_000, 17)
    o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    if S.which == "spheres":
        from test_oracle_conservative_bvh import _rim_rays
        o3, d3 = _rim_rays(S.kw["B"], 20_000, 9)
        o, d = np.concatenate([o, o3]), np.concatenate([d, d3])
    io, to = osc.cast_many(o, d, O.ACCEL_BVH_CONS, threads=16)
    hit = io >= 0
    print(f"\n{S.which}: {int(hit.sum())} of {len(io)} rays hit something in the oracle's answer")
    assert hit.sum() >= 20_000
    for device in (False, True):
        pt = amber.PathTracer(S.hs["A"], amber.Sensor.default(64, 64), flags=amber.PT_FLAG_DEVICE_BUILD if device else 0)
        assert pt.update_flat(0, S.rec["B"], amber.UPDATE_REFIT)["mode_used"] == amber.UPDATE_REFIT
        obj, t, _, _ = pt.kat_cast(o, d)
        pt.close()
        assert np.array_equal(obj, io), int((obj != io).sum())
        assert np.array_equal(bits(t)[hit], bits(to)[hit])


# ---- 5: stream order ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["refit", "rebuild"])
@pytest.mark.parametrize("sc", ["spheres"], indirect=True)
def test_a_pass_enqueued_before_the_update_renders_the_old_scene(amber, sc, mode):
    S = sc
    parts = []
    for key, first in (("A", 0), ("B", 8)):
        pt = S.tracer(key)
        pt.render_pass(first, 8)
        parts.append(pt.download())
        pt.close()
    pt = S.tracer("A", device=mode == "rebuild")
    pt.render_pass(0, 8)
    pt.update_flat(0, S.rec["B"], amber.UPDATE_REFIT if mode == "refit" else amber.UPDATE_REBUILD)
    pt.render_pass(8, 8)
    img, rays = pt.download()
    pt.close()
    assert rays == parts[0][1] + parts[1][1]
    assert np.array_equal(bits(img), bits((parts[0][0] + parts[1][0]).astype(np.float32)))


def _light_room():
    """a room whose ceiling and back wall emit, so that more than half of all paths end with a measurement (a record each): create_arrays' keywords"""
    objects = [(0, 0, [-2, 1.6, -2, 2, 1.6, -2, 2, 1.6, 2]), (0, 0, [-2, 1.6, -2, 2, 1.6, 2, -2, 1.6, 2]),              # ceiling, facing down
               (0, 4, [-2, -1, -2, 2, 1.6, -2, -2, 1.6, -2]), (0, 4, [-2, -1, -2, 2, -1, -2, 2, 1.6, -2]),              # back wall, facing the lens
               (0, 1, [-2, -1, -2, 2, -1, 2, 2, -1, -2]), (0, 1, [-2, -1, -2, -2, -1, 2, 2, -1, 2]),                    # floor
               (1, 2, [0.7, -0.5, 0.1, 0.5]), (1, 3, [-0.8, -0.55, 0.3, 0.45]), (1, 1, [0.0, 0.8, -0.2, 0.3]),
               (2, 1, [-1.8, 0.2, 0.0, 1.0, 0.0, 0.0, 0.8]), (3, 1, [1.4, -1.0, -1.0, 0.0, 1.0, 0.0, 0.2, 1.1])]
    params = np.zeros((len(objects), 12), np.float32)
    for i, (_, _, p) in enumerate(objects):
        params[i, :len(p)] = p
    return dict(kinds=np.array([o[0] for o in objects], np.uint32), material_index=np.array([o[1] for o in objects], np.uint32), params=params,
                materials=[(4, (3.0, 2.0, 1.0), 0.0), (0, (0.7, 0.7, 0.7), 0.0), (2, (0.9, 0.9, 0.9), 0.0), (3, (1.0, 1.0, 1.0), 1.5), (4, (0.5, 1.5, 2.5), 0.0)],
                transform=[1, 0, 0, 0, 0, 1, 0, 0.1, 0, 0, 1, 3.2, 0, 0, 0, 1], focal_length=0.05, focus_distance=3.2, radius=0.02, n_blades=6)


def test_an_update_behind_a_pass_that_has_to_be_repeated(amber):
    """The case the stream order is about: the pass in front of the update ran out of record slots (AMBER_TEST_RECORD_DENSITY_SCALE, the existing
    test hook, mis-sizes its buffer), so the HOST has to repeat it -- and must do so on the OLD scene, before the update touches any array.  A
    shallow tree (a small room through ENGINE_BVH: depth <= 12) renders with the path-granular kernel, whose launches work that way."""
    kw_a = _light_room()
    kw_b = moved(kw_a, 101)
    hs = {"A": amber.HostScene.create_arrays(**kw_a), "B": amber.HostScene.create_arrays(**kw_b)}
    sensor, seed = amber.Sensor.default(640, 512), 11
    parts = []
    for key, passes in (("A", ((0, 8), (8, 56))), ("B", ((64, 8),))):
        pt = amber.PathTracer(hs[key], sensor, seed=seed, engine=amber.ENGINE_BVH)
        for first, n in passes:
            pt.render_pass(first, n)
        parts.append(pt.download())
        pt.close()
    for mode in (amber.UPDATE_REFIT, amber.UPDATE_REBUILD):
        os.environ["AMBER_TEST_RECORD_DENSITY_SCALE"] = "0.02"              # read once, at create: pretend the measured density was 50x lower
        try:
            pt = amber.PathTracer(hs["A"], sensor, seed=seed, engine=amber.ENGINE_BVH)
        finally:
            os.environ.pop("AMBER_TEST_RECORD_DENSITY_SCALE", None)
        assert pt.build_info()["depth"] <= 12                              # include/amber_hip.h: such a tree renders with pt_megakernel<ENGINE_BVH>
        pt.render_pass(0, 8)
        pt.render_pass(8, 56)                                               # seven times the probe's paths, more than half of them with a record, in the probe's
                                                                            # buffer (the mis-sized estimate asks for no larger one): runs out of slots; nobody has looked yet
        pt.update_flat(0, _objects(hs["B"]), mode)
        pt.render_pass(64, 8)
        img, rays = pt.download()
        n_launch, _ = pt.kernel_time()
        pt.close()
        assert n_launch >= 4, n_launch                                      # probe, the failed launch, its repetition, the pass on B
        assert rays == parts[0][1] + parts[1][1]
        assert np.array_equal(bits(img), bits((parts[0][0] + parts[1][0]).astype(np.float32))), mode


# ---- 6: errors leave the handle alone ----------------------------------------------------------------------------------------------------------------
def test_refused_engines_say_to_re_create(amber):
    hs = amber.HostScene.cornell_box()
    rec = _objects(hs)
    for kw in (dict(), dict(engine=amber.ENGINE_LIST), dict(engine=amber.ENGINE_REFERENCE_BVH)):
        pt = amber.PathTracer(hs, amber.Sensor.default(64, 64), seed=2, **kw)
        pt.render_pass(0, 8); before = pt.download()
        for mode in (amber.UPDATE_REFIT, amber.UPDATE_REBUILD):
            with pytest.raises(amber.AmberError, match="re-create"):
                pt.update_flat(0, rec, mode)
        pt.clear(); pt.render_pass(0, 8); after = pt.download()
        pt.close()
        assert before[1] == after[1] and np.array_equal(bits(before[0]), bits(after[0]))


@pytest.mark.parametrize("sc", ["spheres"], indirect=True)
def test_errors_leave_the_handle_alone(amber, sc):
    S = sc
    n = len(S.rec["A"])
    pt = S.tracer("A", device=True)
    zero = pt.update_flat(0, S.rec["B"][:0])                                # count == 0 on a fresh handle: OK, and the figures are those of the tree in use
    assert zero["area_before"] == zero["area_after"] > 1 and zero["n_nodes"] == pt.build_info()["n_nodes"], zero
    want = S.band(pt)
    dump = pt.bvh_dump()
    B = S.rec["B"]

    def bad(first, rec, mode=amber.UPDATE_REFIT, match=None, count=None):
        with pytest.raises(amber.AmberError, match=match):
            pt.update_flat(first, rec, mode, count=count)
        assert _same_dump(pt.bvh_dump(), dump)
        pt.clear()
        got = S.band(pt)
        assert got[1] == want[1] and np.array_equal(got[0], want[0]), match

    bad(n - 3, B[:4], match="not all in the scene")                        # range past the end
    bad(n + 1, B[:0], match="not all in the scene", count=0)
    bad(10, None, match="null objects", count=4)
    bad(0, B, mode=7, match="unknown mode")
    for mode in (amber.UPDATE_REFIT, amber.UPDATE_REBUILD):
        rec = B.copy(); rec["kind"][1000] = 2
        bad(0, rec, mode, match="object 1000: kind or material")
        rec = B.copy(); rec["material"][2000] ^= 1; rec["material"][3000] ^= 1
        bad(1500, rec[1500:], mode, match="object 2000: kind or material")
        blade = int(S.blades[min(2, S.n_blades - 1)])
        rec = B.copy(); rec["p"][blade, 4] += np.float32(1e-3)
        bad(0, rec, mode, match=f"object {blade} is an aperture blade")
        rec = B.copy(); rec["p"][777, 1] = np.inf
        bad(0, rec, mode, match="no finite bounds")
    assert pt.update_flat(5, B[:0])["mode_used"] == amber.UPDATE_REFIT      # count == 0: OK, nothing changes
    assert pt.update_flat(n, None, count=0)["n_nodes"] == len(dump["nodes"])
    assert _same_dump(pt.bvh_dump(), dump)
    pt.close()


@pytest.mark.parametrize("sc", ["spheres"], indirect=True)
def test_lights_go_stale_only_when_a_lights_object_changes(amber, sc):
    S = sc
    A, B = S.rec["A"], S.rec["B"]
    emit = np.array([S.kw["A"]["materials"][m][0] == MAT_DIFFUSE_LIGHT for m in np.asarray(S.kw["A"]["material_index"])])   # (the six blades come first)
    assert len(emit) == len(S.user)
    assert 100 < emit.sum() < len(emit)
    sensor = amber.Sensor.default(64, 48)
    pt = amber.PathTracer(S.hs["A"], sensor, seed=3)
    want = pt.lt_trace(0, 8)
    assert pt.update_flat(0, A)["mode_used"] == amber.UPDATE_REFIT          # blades and lights in the range, records unchanged
    got = pt.lt_trace(0, 8)
    assert got[1] == want[1] > 0 and got[0].tobytes() == want[0].tobytes()
    rec = A.copy()                                                          # only the objects that emit nothing move: the lights table still holds
    rec[S.user[~emit]] = B[S.user[~emit]]
    pt.update_flat(0, rec)
    assert pt.lt_trace(0, 8)[1] > 0
    pt.update_flat(0, B)                                                    # now the emitting spheres move too
    with pytest.raises(amber.AmberError, match="lights are stale after amber_hip_pt_update_objects: re-create the handle"):
        pt.lt_trace(0, 8)
    pt.close()
    pt = S.tracer("A")
    pt.update_flat(0, B)
    img, rays = S.band(pt)
    pt.close()
    assert rays == S.fresh("B")[1] and np.array_equal(img, S.fresh("B")[0])   # path tracing does not read the lights table


def test_a_scene_with_nan_objects_as_the_target_of_an_update(amber):
    """validate_tree cannot judge this scene -- the padded box it computes for an object with a NaN parameter is NaN, which no leaf box of any tree
    contains by its comparisons -- so the tree is held to what it can be held to: every object once in the leaf order, the topology untouched by a
    refit, every plane finite and inside the grid's reach, and the closest hits of 100 000 rays those of the plain scan over all objects."""
    kw_b = _nan_scene()
    kw_a = dict(kw_b, params=np.nan_to_num(kw_b["params"], nan=0.01))
    hs_a, hs_b = amber.HostScene.create_arrays(**kw_a), amber.HostScene.create_arrays(**kw_b)
    rec = _objects(hs_b)
    assert np.isnan(rec["p"][:, :4]).any(axis=1).sum() > 100
    W, H, rows = 512, 512, (240, 272)
    pt = amber.PathTracer(hs_b, amber.Sensor.default(W, H), seed=9, rows=rows)
    pt.render_pass(0, 16); want, want_rays = pt.download(); pt.close()
    assert bits(want).any()
    o, d = _random_rays(rec[~np.isnan(rec["p"][:, :4]).any(axis=1)], 100_000, 23)
    pt = amber.PathTracer(hs_b, amber.Sensor.default(64, 64), engine=amber.ENGINE_LIST)
    list_obj, list_t, _, _ = pt.kat_cast(o, d)
    pt.close()
    assert (list_obj >= 0).sum() > 30_000
    for device, mode in ((False, amber.UPDATE_REFIT), (True, amber.UPDATE_REFIT), (False, amber.UPDATE_REBUILD)):
        pt = amber.PathTracer(hs_a, amber.Sensor.default(W, H), seed=9, rows=rows, flags=amber.PT_FLAG_DEVICE_BUILD if device else 0)
        before = pt.bvh_dump()
        info = pt.update_flat(0, rec, mode)
        dump = pt.bvh_dump()
        assert info["mode_used"] == mode and info["n_nodes"] == len(dump["nodes"])
        assert np.array_equal(np.sort(dump["prims"]), np.arange(len(rec)))
        f16 = (np.concatenate([dump["nodes"][:, :6] & 0xffff, dump["nodes"][:, :6] >> 16]).astype(np.uint16)).view(np.float16).astype(np.float64)
        assert np.isfinite(f16).all()
        if mode == amber.UPDATE_REFIT:
            _decode(dump)                                                    # a refit's planes: never a binary16 denormal, inside the reach
            assert dump["nodes"][:, 6:8].tobytes() == before["nodes"][:, 6:8].tobytes() and dump["prims"].tobytes() == before["prims"].tobytes()
        obj, t, _, _ = pt.kat_cast(o, d)
        assert np.array_equal(obj, list_obj) and np.array_equal(bits(t)[list_obj >= 0], bits(list_t)[list_obj >= 0])
        pt.render_pass(0, 16); img, rays = pt.download(); pt.close()
        assert rays == want_rays and np.array_equal(bits(img), bits(want)), (device, mode)


# ---- 7: a REBUILD that cannot be used refits ------------------------------------------------------------------------------------------------------------
DEPTH_CHILD = r"""
import os, sys, json
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import amber_amd as A
from amber_amd import scenes
from test_update_objects import moved
from test_device_build import _objects
kw = scenes.random_spheres(20_000, 7)
hs_a, hs_b = A.HostScene.create_arrays(**kw), A.HostScene.create_arrays(**moved(kw, 101))
pt = A.PathTracer(hs_b, A.Sensor.default(256, 256), seed=4, rows=(120, 136))
pt.render_pass(0, 16); want, want_rays = pt.download(); pt.close()
pt = A.PathTracer(hs_a, A.Sensor.default(256, 256), seed=4, rows=(120, 136))
before, build = pt.bvh_dump(), pt.build_info()
info = pt.update_flat(0, _objects(hs_b), A.UPDATE_REBUILD)
after = pt.bvh_dump()
pt.render_pass(0, 16); img, rays = pt.download()
same_topology = before["nodes"][:, 6:8].tobytes() == after["nodes"][:, 6:8].tobytes() and before["prims"].tobytes() == after["prims"].tobytes()
print("RESULT " + json.dumps(dict(info=info, same_topology=bool(same_topology), same_image=bool(rays == want_rays and img.tobytes() == want.tobytes()),
                                  build_unchanged=bool(pt.build_info() == build), where=build["where"])))
pt.close()
"""


def test_a_rebuild_deeper_than_the_limit_refits_the_tree_in_use(amber):
    env = dict(os.environ, AMBER_TEST_DEVICE_BUILD_MAX_DEPTH="6")
    p = subprocess.run([sys.executable, "-c", DEPTH_CHILD.format(root=str(ROOT))], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    assert res["where"] == amber.BUILD_HOST
    assert res["info"]["mode_used"] == amber.UPDATE_REFIT and res["info"]["fallback_reason"] == amber.BUILD_REASON_DEPTH, res
    assert res["same_topology"] and res["same_image"] and res["build_unchanged"], res


# ---- 8: no growth ------------------------------------------------------------------------------------------------------------------------------------
GROWTH_CHILD = r"""
import os, sys, json
import torch
torch.cuda.init()                                        # (before the engine's library: the measurement needs torch's runtime up)
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import amber_amd as A
from amber_amd import scenes
from test_update_objects import moved
from test_device_build import _objects
kw = scenes.random_spheres(50_000, 7)
hs = dict(A=A.HostScene.create_arrays(**kw), B=A.HostScene.create_arrays(**moved(kw, 101)))
rec = {{k: _objects(h) for k, h in hs.items()}}
out = {{}}
for mode in (A.UPDATE_REFIT, A.UPDATE_REBUILD):
    pt = A.PathTracer(hs["A"], A.Sensor.default(256, 256), seed=4, rows=(120, 136))
    free = []
    for k in range(20):
        pt.update_flat(0, rec["AB"[(k + 1) % 2]], mode)
        pt.render_pass(0, 8); pt.sync()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    pt.close()
    out[str(mode)] = free
print("RESULT " + json.dumps(out))
"""


def test_twenty_updates_do_not_grow_device_memory(amber):
    """20 full-range updates alternating B / A in each mode: free device memory after update 20 is not lower than after update 3.  (In a child process:
    torch.cuda.mem_get_info needs torch's runtime initialised before the engine's library is loaded.)"""
    p = subprocess.run([sys.executable, "-c", GROWTH_CHILD.format(root=str(ROOT))], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    for mode, free in res.items():
        print(f"\nmode {mode}: free device memory after updates 3 and 20: {free[2]} {free[19]}")
        assert len(free) == 20 and free[19] >= free[2], (mode, free)


# ---- 9: faster than what it replaces -------------------------------------------------------------------------------------------------------------------
def test_an_update_is_faster_than_destroy_and_create(amber):
    """Medians of 5 after a warm-up of each kind, every step timed to a sync.  destroy + create(DEVICE_BUILD) is the parent commit's shortest route to the same state."""
    for name, kw in (("1M spheres", scenes.random_spheres(1_000_000, 7)), ("terrain", WL.terrain_mesh(16, 56).arrays())):
        hs = {"A": amber.HostScene.create_arrays(**kw), "B": amber.HostScene.create_arrays(**moved(kw, 101))}
        rec = {k: _objects(h) for k, h in hs.items()}
        sensor = amber.Sensor.default(64, 64)
        med = {}
        pt = amber.PathTracer(hs["A"], sensor, flags=amber.PT_FLAG_DEVICE_BUILD)
        times = []
        for k in range(6):                                                  # the first one is the warm-up
            t0 = time.perf_counter()
            pt.close()
            pt = amber.PathTracer(hs["AB"[(k + 1) % 2]], sensor, flags=amber.PT_FLAG_DEVICE_BUILD)
            pt.sync()
            times.append((time.perf_counter() - t0) * 1e3)
        med["create"] = statistics.median(times[1:])
        for mode, label in ((amber.UPDATE_REBUILD, "rebuild"), (amber.UPDATE_REFIT, "refit")):
            times = []
            for k in range(6):
                t0 = time.perf_counter()
                pt.update_flat(0, rec["AB"[(k + 1) % 2]], mode)
                pt.sync()
                times.append((time.perf_counter() - t0) * 1e3)
            med[label] = statistics.median(times[1:])
        pt.close()
        print(f"\n{name}: destroy + create(DEVICE_BUILD) {med['create']:.1f} ms, update REBUILD {med['rebuild']:.1f} ms, update REFIT {med['refit']:.1f} ms")
        assert med["rebuild"] < med["create"] and med["refit"] < med["create"], (name, med)


# ---- 10: the product library ---------------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import os, sys, json
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import amber_amd as A
from amber_amd import scenes
from test_update_objects import moved
assert A.library_path().name == "libamber_hip.so" and not A.is_lab()
kw = scenes.random_spheres(60_000, 7)
hs_a, hs_b = A.HostScene.create_arrays(**kw), A.HostScene.create_arrays(**moved(kw, 101))
objs, _, _ = hs_b.flatten()
rec = np.frombuffer(objs, dtype=np.dtype([("kind", np.uint32), ("material", np.uint32), ("p", np.float32, (12,))])).copy()
out = {{}}
for name, mode, flags in (("refit", A.UPDATE_REFIT, 0), ("rebuild", A.UPDATE_REBUILD, A.PT_FLAG_DEVICE_BUILD)):
    pt = A.PathTracer(hs_a, A.Sensor.default(192, 108), seed=11, rows=(40, 56), flags=flags)
    pt.render_pass(0, 16)
    info = pt.update_flat(0, rec, mode)
    pt.clear(); pt.render_pass(0, 16); img, rays = pt.download(); build = pt.build_info(); pt.close()
    np.save(os.path.join({tmp!r}, name + ".npy"), img)
    out[name] = dict(info=info, rays=int(rays), build=build)
print("RESULT " + json.dumps(out))
"""


def test_product_library_updates_and_renders_the_lab_builds_bits(amber, tmp_path):
    env = dict(os.environ, AMBER_AMD_LIB="libamber_hip.so")
    p = subprocess.run([sys.executable, "-c", CHILD.format(root=str(ROOT), tmp=str(tmp_path))], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    kw = moved(scenes.random_spheres(60_000, 7), 101)
    pt = amber.PathTracer(amber.HostScene.create_arrays(**kw), amber.Sensor.default(192, 108), seed=11, rows=(40, 56))   # the lab build, a fresh handle, the host's tree
    pt.render_pass(0, 16)
    img, rays = pt.download()
    pt.close()
    for name, mode in (("refit", amber.UPDATE_REFIT), ("rebuild", amber.UPDATE_REBUILD)):
        assert res[name]["info"]["mode_used"] == mode and res[name]["info"]["n_nodes"] == res[name]["build"]["n_nodes"] > 10_000, res
        assert rays == res[name]["rays"] and np.array_equal(bits(np.load(tmp_path / (name + ".npy"))), bits(img)), name

"""AMBER_PT_FLAG_DEVICE_BUILD on the GPU: engine BVH's tree built by kernels at create (amber_amd/csrc/hip/bvh_device_build.inc).

The answer of engine BVH does not depend on its tree (exact leaf tests, the (t, lower object index) rule), so a device-built tree has to give
the bits the host-built one gives, and the frozen oracle checks it as it checks the host's: (1) build_info says who built the tree;
(2) a numpy validator proves the dumped tree conservative by the host builder's own formulae -- first on host-built trees, which shows the
validator right; (3) closest hits of path rays and random rays equal oracle(List); (4) the bands of the existing parity tests, with their
frames, seeds, rows, spp and caps, through bvh_parity.check_band; (5) host tree against device tree: image bits, ray counts, path signatures,
light-tracing splats; (6) two builds give identical bytes; (7) create is faster; (8) the product library does the same as the lab build.
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
from bvh_parity import bits, check_band
from tree_reference import pad_boxes, scene_extent, widened_object_boxes

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
K_LEAF, K_MAX_DEPTH = 3, 30                     # bvh_build.h: kLeafSize, kMaxDepth


# ---- the validator -------------------------------------------------------------------------------------------------------------------
def _objects(hs):
    objs, _, _ = hs.flatten()
    return np.frombuffer(objs, dtype=np.dtype([("kind", np.uint32), ("material", np.uint32), ("p", np.float32, (12,))])).copy()


def _padded_object_boxes(arr):
    """bvh_build.h's ObjectBox (widened: sphere slack 16 eps D^2, needle reach) and PadBox of every object, with the roundings of the C++ code:
    tree_reference.widened_object_boxes, then tree_reference.pad_boxes with the extent of the scene (binary32), as binary64."""
    mn, mx = widened_object_boxes(arr)
    mn, mx = pad_boxes(mn, mx, scene_extent(mn, mx))
    return mn.astype(np.float64), mx.astype(np.float64)


def _decode(dump):
    """(lo, hi): (n, 2, 3) float64 planes of the left / right child box of every node; (n, 2) int32 child references."""
    nodes = dump["nodes"]
    w = nodes[:, :6].reshape(-1, 2, 3)
    f16 = lambda half: half.astype(np.uint16).view(np.float16).astype(np.float64)
    vlo, vhi = f16(w & 0xffff), f16(w >> 16)
    assert np.isfinite(vlo).all() and np.isfinite(vhi).all()
    for v in (vlo, vhi):                                                    # never a binary16 denormal; inside the reach
        assert ((v == 0) | (np.abs(v) >= 2.0 ** -14)).all() and (np.abs(v) <= 1.0 + 2.0 ** -10).all()
    g, s = dump["gmin"].astype(np.float64), dump["step"].astype(np.float64)
    return g + vlo * s, g + vhi * s, nodes[:, 6:8].view(np.int32)


def validate_tree(dump, arr, label=""):
    n_obj = len(arr)
    omn, omx = _padded_object_boxes(arr)
    prims = dump["prims"].astype(np.int64)
    assert len(prims) == n_obj and np.array_equal(np.sort(prims), np.arange(n_obj)), label          # every object exactly once in the leaf order
    kind = arr["kind"][prims]
    seen = np.zeros(n_obj, np.int64)

    def check_leaves(refs, lo, hi):
        r = -(refs.astype(np.int64) + 1)
        first, count, tris, sph = r >> 4, r & 3, (r & 8) != 0, (r & 4) != 0
        assert ((count >= 1) & (count <= K_LEAF)).all() and (first + count <= n_obj).all() , label
        for k in range(K_LEAF):
            sel = count > k
            slot = (first + k)[sel]
            np.add.at(seen, slot, 1)
            obj = prims[slot]
            if lo is not None:
                assert (lo[sel] <= omn[obj]).all() and (hi[sel] >= omx[obj]).all(), (label, "a leaf box does not contain its object's padded box")
        all_t, all_s = np.ones(len(r), bool), np.ones(len(r), bool)
        for k in range(K_LEAF):
            sel = count > k
            kk = kind[np.minimum(first + k, n_obj - 1)]
            all_t &= ~sel | (kk == 0); all_s &= ~sel | (kk == 1)
        assert np.array_equal(all_t, tris) and np.array_equal(all_s, sph), (label, "kind bits of a leaf")

    if len(dump["nodes"]) == 0:
        assert dump["root"] < 0 and dump["depth"] == 0, label
        check_leaves(np.array([dump["root"]], np.int32), None, None)
        assert (seen == 1).all(), label
        return dict(nodes=0, depth=0)
    lo, hi, child = _decode(dump)
    assert dump["root"] == 0, label
    reached = np.zeros(len(child), bool)
    frontier, depth = np.array([0], np.int64), 0
    while len(frontier):
        assert not reached[frontier].any(), (label, "a node has two parents")
        reached[frontier] = True
        depth += 1
        assert depth <= K_MAX_DEPTH, (label, "deeper than the traversal's limit")
        nxt = []
        for side in (0, 1):
            ref = child[frontier, side]
            leaf = ref < 0
            check_leaves(ref[leaf], lo[frontier[leaf], side], hi[frontier[leaf], side])
            par, kid = frontier[~leaf], ref[~leaf].astype(np.int64)
            assert (kid < len(child)).all(), label
            # the box the parent keeps for an inner child contains both boxes stored in the child
            assert (lo[par, side][:, None, :] <= lo[kid]).all() and (hi[par, side][:, None, :] >= hi[kid]).all(), (label, "a child box does not contain its grandchildren")
            nxt.append(kid)
        frontier = np.concatenate(nxt)
    assert reached.all(), (label, "unreachable nodes")
    assert (seen == 1).all(), (label, "an object is in no leaf, or in two")
    assert depth == dump["depth"], (label, depth, dump["depth"])
    return dict(nodes=len(child), depth=depth)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def _mixed_scene(n=3000, seed=11):
    rng = np.random.default_rng(seed)
    kinds = rng.integers(0, 4, n).astype(np.uint32)
    params = np.zeros((n, 12), np.float32)
    c = rng.uniform(-1, 1, (n, 3))
    params[:, :3] = c
    t = kinds == 0
    params[t, 3:6] = (c + rng.normal(size=(n, 3)) * 0.03)[t]; params[t, 6:9] = (c + rng.normal(size=(n, 3)) * 0.03)[t]
    params[kinds == 1, 3] = rng.uniform(0.005, 0.03, (kinds == 1).sum())
    nrm = rng.normal(size=(n, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[::7] *= 0.5                                                        # non-unit cylinder axes / disk normals too
    for k in (2, 3):
        params[kinds == k, 3:6] = nrm[kinds == k]
        params[kinds == k, 6] = rng.uniform(0.005, 0.03, (kinds == k).sum())
    params[kinds == 3, 7] = rng.uniform(0.01, 0.08, (kinds == 3).sum())
    kw = scenes.random_spheres(4, 1)
    return dict(kw, kinds=kinds, material_index=rng.integers(0, 4, n).astype(np.uint32), params=params)


def _planar_scene(n=4000, offset=1234.5, seed=5):
    """a mesh without any extent in z, far from the origin (pinhole lens in the same plane: no object anywhere else)"""
    rng = np.random.default_rng(seed)
    params = np.zeros((n, 12), np.float32)
    c = rng.uniform(-2, 2, (n, 2))
    for v in range(3):
        params[:, 3 * v:3 * v + 2] = c + rng.normal(size=(n, 2)) * 0.02
        params[:, 3 * v + 2] = offset
    kw = scenes.random_spheres(4, 1)
    return dict(kw, kinds=np.zeros(n, np.uint32), material_index=np.ones(n, np.uint32), params=params,
                transform=[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, offset, 0, 0, 0, 1], n_blades=0)


def _coincident_scene(n=2000):
    kw = scenes.random_spheres(n, 3)
    kw["params"][:, :3] = np.float32([0.25, -0.5, 0.125])
    return kw


def _three_objects():
    kw = scenes.random_spheres(2, 3)
    return dict(kw, n_blades=0)                                               # the pinhole's aperture triangle + two spheres


@pytest.fixture(scope="module")
def spheres(amber):
    kw = scenes.random_spheres(50_000, 7)
    return amber.HostScene.create_arrays(**kw), O.Scene.create_arrays(**kw, accel=O.ACCEL_BVH_CONS)


@pytest.fixture(scope="module")
def room(amber, tmp_path_factory):
    wl = WL.room_mesh(3)
    return amber.HostScene.import_file(wl.write(tmp_path_factory.mktemp("room"))), O.Scene.create_arrays(**wl.arrays(), accel=O.ACCEL_BVH_CONS | O.BLADES_LAST)


@pytest.fixture(scope="module")
def terrain(amber, tmp_path_factory):
    wl = WL.terrain_mesh(16, 56)
    return amber.HostScene.import_file(wl.write(tmp_path_factory.mktemp("terrain"))), O.Scene.create_arrays(**wl.arrays(), accel=O.ACCEL_BVH_CONS | O.BLADES_LAST)


@pytest.fixture(scope="module")
def config3(amber):
    kw = scenes.random_spheres(1_000_000, 7)
    return amber.HostScene.create_arrays(**kw), O.Scene.create_arrays(**kw, accel=O.ACCEL_BVH_CONS)


def _tracer(amber, hs, device, W=64, H=64, **kw):
    flags = kw.pop("flags", 0) | (amber.PT_FLAG_DEVICE_BUILD if device else 0)
    return amber.PathTracer(hs, amber.Sensor.default(W, H), flags=flags, **kw)


# ---- 1: where the tree was built ---------------------------------------------------------------------------------------------------------
def test_build_info_says_where_the_tree_was_built(amber, spheres):
    hs = spheres[0]
    for device, where in ((True, amber.BUILD_DEVICE), (False, amber.BUILD_HOST)):
        pt = _tracer(amber, hs, device)
        info, dump = pt.build_info(), pt.bvh_dump()
        pt.close()
        assert info["where"] == where and info["fallback_reason"] == 0, info
        assert info["n_nodes"] == len(dump["nodes"]) > 10_000 and info["depth"] == dump["depth"] > 10 and info["n_leaves"] == info["n_nodes"] + 1
        assert 0 < info["tree_ms"] <= info["create_ms"]
    for device in (True, False):                                            # the Cornell box under AUTO: the two-phase engine, no tree; the flag is accepted
        pt = _tracer(amber, amber.HostScene.cornell_box(), device)
        info = pt.build_info()
        pt.close()
        assert info["where"] == amber.BUILD_NONE and info["n_nodes"] == 0 and info["create_ms"] > 0, info


# ---- 2: the tree is conservative ---------------------------------------------------------------------------------------------------------
def test_device_built_trees_are_valid_by_the_host_builders_rules(amber, spheres, room, terrain):
    cases = [("50 000 spheres", spheres[0], {}), ("Cornell through ENGINE_BVH", amber.HostScene.cornell_box(), dict(engine=amber.ENGINE_BVH)),
             ("room mesh", room[0], {}), ("terrain", terrain[0], {}), ("disks and cylinders", amber.HostScene.create_arrays(**_mixed_scene()), {}),
             ("planar mesh at z = 1234.5", amber.HostScene.create_arrays(**_planar_scene()), {}),
             ("3 objects", amber.HostScene.create_arrays(**_three_objects()), dict(engine=amber.ENGINE_BVH)),
             ("2 000 spheres with one centre", amber.HostScene.create_arrays(**_coincident_scene()), {})]
    for name, hs, kw in cases:
        arr = _objects(hs)
        for device in (False, True):                                         # the host's tree first: the validator must accept it
            pt = _tracer(amber, hs, device, **kw)
            info, dump = pt.build_info(), pt.bvh_dump()
            pt.close()
            if device and info["where"] == amber.BUILD_HOST_FALLBACK:        # allowed where the Morton tree is too deep -- and then the host's tree is in use
                assert name.startswith("2 000") and info["fallback_reason"] == amber.BUILD_REASON_DEPTH, (name, info)
            else:
                assert info["where"] == (amber.BUILD_DEVICE if device else amber.BUILD_HOST), (name, info)
            st = validate_tree(dump, arr, f"{name}, {'device' if device else 'host'}")
            assert st["nodes"] == info["n_nodes"] and st["depth"] == info["depth"]
            print(f"\n{name}: {'device' if device else 'host'} tree of {len(arr)} objects: {st['nodes']} nodes, depth {st['depth']} (where = {info['where']})")
        if name == "3 objects":
            assert st["nodes"] == 0
        if name == "Cornell through ENGINE_BVH":
            assert st["depth"] <= 8


# ---- 3: closest hits -----------------------------------------------------------------------------------------------------------------------
def _random_rays(arr, n, seed):
    rng = np.random.default_rng(seed)
    c = arr["p"][:, :3]
    lo, hi = np.nanmin(c, 0) - 0.5, np.nanmax(c, 0) + 0.5
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    target = c[rng.integers(0, len(c), n)] + rng.normal(size=(n, 3)) * 0.02
    d = target - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return o, d


@pytest.mark.parametrize("which", ["spheres", "room", "terrain"])
def test_closest_hits_of_the_device_built_tree_equal_the_list_oracle(amber, request, which):
    hs, osc = request.getfixturevalue(which)
    W, H, seed, rows = {"spheres": (1024, 1024, 7, (500, 503)), "room": (1024, 1024, 7, (650, 653)), "terrain": (1920, 1080, 3, (810, 812))}[which]
    osc.set_accel(O.ACCEL_BVH_CONS)
    o1, d1 = osc.collect_rays(W, H, seed, 0, 2, rows, 40_000)
    o2, d2 = _random_rays(_objects(hs), 100_000, 17)
    o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    if which == "spheres":
        from test_oracle_conservative_bvh import _rim_rays
        o3, d3 = _rim_rays(scenes.random_spheres(50_000, 7), 20_000, 9)
        o, d = np.concatenate([o, o3]), np.concatenate([d, d3])
    io, to = osc.cast_many(o, d, O.ACCEL_BVH_CONS, threads=16)
    pt = _tracer(amber, hs, True)
    assert pt.build_info()["where"] == amber.BUILD_DEVICE
    obj, t, _, _ = pt.kat_cast(o, d)
    pt.close()
    hit = io >= 0
    assert hit.sum() > 20_000
    assert np.array_equal(obj, io), int((obj != io).sum())
    assert np.array_equal(bits(t)[hit], bits(to)[hit])


# ---- 4: bands against the oracle, with the existing tests' frames, seeds, rows, spp and caps -----------------------------------------------
def test_cornell_band_through_a_device_built_tree(amber, oracle):
    hs, osc = amber.HostScene.cornell_box(), O.Scene.cornell(O.ACCEL_BVH_CONS)
    for flags, name in ((0, "Cornell, device tree, pt_megakernel<ENGINE_BVH>"), (amber.PT_FLAG_BVH_ITEMS, "Cornell, device tree, pt_bvh_megakernel")):
        check_band(amber, hs, osc, 1024, 1024, 12345, 64, (600, 632), max_ref_pixels=8, max_ref_ray_delta=64, engine=amber.ENGINE_BVH, flags=flags | amber.PT_FLAG_DEVICE_BUILD, label=name)


def test_room_mesh_band_through_a_device_built_tree(amber, room):
    for flags, name in ((0, "room mesh, device tree"), (amber.PT_FLAG_BVH_ITEMS, "room mesh, device tree, pt_bvh_megakernel")):
        st = check_band(amber, room[0], room[1], 1024, 1024, 7, 64, (640, 672), max_ref_pixels=32, max_ref_ray_delta=256, flags=flags | amber.PT_FLAG_DEVICE_BUILD, label=name)
        assert st["lit"] > 0.25


def test_terrain_band_through_a_device_built_tree(amber, terrain):
    st = check_band(amber, terrain[0], terrain[1], 1920, 1080, 3, 32, (800, 824), max_ref_pixels=256, max_ref_ray_delta=2048, flags=amber.PT_FLAG_DEVICE_BUILD, label="terrain, device tree")
    assert st["lit"] > 0.25


def test_config3_band_through_a_device_built_tree(amber, config3):
    check_band(amber, config3[0], config3[1], 1920, 1080, 1, 256, (508, 572), max_ref_pixels=32, max_ref_ray_delta=512, flags=amber.PT_FLAG_DEVICE_BUILD, label="config 3, device tree")


# ---- 5: host tree against device tree ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["spheres", "room", "terrain"])
def test_host_and_device_trees_render_the_same_bits(amber, request, which):
    hs, _ = request.getfixturevalue(which)
    W, H, seed, rows, spp = {"spheres": (1024, 1024, 7, (500, 516), 16), "room": (1024, 1024, 7, (640, 656), 16), "terrain": (1920, 1080, 3, (800, 816), 8)}[which]
    got = []
    for device in (False, True):
        pt = _tracer(amber, hs, device, W, H, seed=seed, rows=rows)
        assert pt.build_info()["where"] == (amber.BUILD_DEVICE if device else amber.BUILD_HOST)
        pt.render_pass(0, spp)
        img, rays = pt.download()
        pt.close()
        pt = _tracer(amber, hs, device, W, H, seed=seed, rows=(rows[0], rows[0] + 4))
        sig = pt.render_signatures(0, 8)
        pt.close()
        got.append((bits(img).copy(), rays, sig))
    assert got[0][1] == got[1][1] and np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][2], got[1][2])
    if which == "room":
        splats = []
        for device in (False, True):
            pt = _tracer(amber, hs, device, 64, 48, seed=3)
            splats.append(pt.lt_trace(0, 16))
            pt.close()
        a, b = splats
        assert a[1] == b[1] > 0 and a[0].tobytes() == b[0].tobytes()


def _nan_scene(n=4000, seed=5):
    """spheres of which every 37th has a NaN centre coordinate, a NaN radius, or both: create accepts them, no ray hits them (every root of a NaN
    discriminant is NaN), and their NaN bounds must not reach any box of the tree"""
    kw = scenes.random_spheres(n, seed)
    params, mat = kw["params"], kw["material_index"]
    bad = np.arange(5, n, 37)
    mat[bad] = 1                                                            # never a light: its power would be NaN
    for j, i in enumerate(bad):
        if j % 3 != 1:
            params[i, j % 3] = np.nan
        if j % 3 != 0:
            params[i, 3] = np.nan
    return kw


def test_objects_with_nan_bounds_do_not_poison_the_device_built_tree(amber):
    """A NaN centre or radius makes an object's box NaN.  The host builder skips such bounds (reset, then grow with the accumulator first); the device's
    bottom-up pass must do the same whichever thread arrives first: finite neighbours stay hittable, and the tree does not depend on the arrival order."""
    kw = _nan_scene()
    hs = amber.HostScene.create_arrays(**kw)
    arr = _objects(hs)
    assert np.isnan(arr["p"][:, :4]).any(axis=1).sum() > 100
    o, d = _random_rays(arr[~np.isnan(arr["p"][:, :4]).any(axis=1)], 100_000, 23)
    W, H, rows = 512, 512, (240, 272)
    got, dumps = [], []
    pt = amber.PathTracer(hs, amber.Sensor.default(64, 64), engine=amber.ENGINE_LIST)     # the plain scan over all objects: what every tree has to give
    list_obj, list_t, _, _ = pt.kat_cast(o, d)
    pt.close()
    for device in (False, True, True, True):
        pt = _tracer(amber, hs, device, W, H, seed=9, rows=rows)
        assert pt.build_info()["where"] == (amber.BUILD_DEVICE if device else amber.BUILD_HOST)
        if device:
            dumps.append(pt.bvh_dump())
        pt.render_pass(0, 16)
        img, rays = pt.download()
        obj, t, _, _ = pt.kat_cast(o, d)
        pt.close()
        got.append((bits(img).copy(), rays, obj, bits(t).copy()))
    assert (got[0][2] >= 0).sum() > 30_000 and got[0][0].any()
    assert np.array_equal(got[0][2], list_obj) and np.array_equal(got[0][3][list_obj >= 0], bits(list_t)[list_obj >= 0])
    for g in got[1:]:
        assert g[1] == got[0][1] and np.array_equal(g[0], got[0][0]), "image of the device tree differs from the host tree's"
        hit = got[0][2] >= 0
        assert np.array_equal(g[2], got[0][2]) and np.array_equal(g[3][hit], got[0][3][hit]), "closest hits differ"
    for dmp in dumps[1:]:
        for key in ("nodes", "prims", "gmin", "step", "reach"):
            assert dmp[key].tobytes() == dumps[0][key].tobytes(), key
    # no plane word of the tree decodes to NaN or infinity
    nodes = dumps[0]["nodes"]
    f16 = (np.concatenate([nodes[:, :6] & 0xffff, nodes[:, :6] >> 16]).astype(np.uint16)).view(np.float16).astype(np.float64)
    assert np.isfinite(f16).all()


# ---- the host fallback from inside create --------------------------------------------------------------------------------------------------
FALLBACK_CHILD = r"""
import os, sys, json
sys.path.insert(0, {root!r})
import numpy as np
import amber_amd as A
from amber_amd import scenes
hs = A.HostScene.create_arrays(**scenes.random_spheres(20_000, 7))
out = {{}}
for name, flags in (("host", 0), ("flag", A.PT_FLAG_DEVICE_BUILD)):
    pt = A.PathTracer(hs, A.Sensor.default(256, 256), seed=4, rows=(120, 136), flags=flags)
    info, dump = pt.build_info(), pt.bvh_dump(); pt.render_pass(0, 16); img, rays = pt.download(); pt.close()
    np.save(os.path.join({tmp!r}, name + ".npy"), img); np.save(os.path.join({tmp!r}, name + "_nodes.npy"), dump["nodes"]); np.save(os.path.join({tmp!r}, name + "_prims.npy"), dump["prims"])
    out[name] = dict(info=info, rays=int(rays), depth=dump["depth"])
print("RESULT " + json.dumps(out))
"""


def _fallback_child(tmp_path, env):
    p = subprocess.run([sys.executable, "-c", FALLBACK_CHILD.format(root=str(ROOT), tmp=str(tmp_path))], capture_output=True, text=True, env=dict(os.environ, **env), timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    for part in (".npy", "_nodes.npy", "_prims.npy"):                       # the fallback's tree IS the host's tree, and renders its bits
        assert np.load(tmp_path / ("host" + part)).tobytes() == np.load(tmp_path / ("flag" + part)).tobytes(), part
    assert res["host"]["rays"] == res["flag"]["rays"] and res["host"]["info"]["where"] == 1
    for key in ("n_nodes", "n_leaves", "depth"):
        assert res["host"]["info"][key] == res["flag"]["info"][key]
    return res


def test_a_tree_deeper_than_the_limit_is_replaced_by_the_hosts(amber, tmp_path):
    """AMBER_TEST_DEVICE_BUILD_MAX_DEPTH (a test hook) lowers the depth the device build accepts, so that create's fallback -- the host builder called
    after the scene's state has moved into the handle -- runs on an ordinary scene: HOST_FALLBACK with the depth reason, the host's tree, the host's bits."""
    res = _fallback_child(tmp_path, dict(AMBER_TEST_DEVICE_BUILD_MAX_DEPTH="6"))
    info = res["flag"]["info"]
    assert info["where"] == amber.BUILD_HOST_FALLBACK and info["fallback_reason"] == amber.BUILD_REASON_DEPTH and info["depth"] > 6, info
    assert info["tree_ms"] > res["host"]["info"]["tree_ms"] * 0.5


def test_the_four_wide_build_falls_back_to_the_host_builder(amber, tmp_path):
    subprocess.run(["make", "-C", str(ROOT / "amber_amd" / "csrc"), "wide"], check=True, capture_output=True, timeout=900)
    res = _fallback_child(tmp_path, dict(AMBER_AMD_LIB="libamber_hip_wide.so"))
    info = res["flag"]["info"]
    assert info["where"] == amber.BUILD_HOST_FALLBACK and info["fallback_reason"] == amber.BUILD_REASON_WIDE, info


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
def test_command_line_with_device_build_writes_the_same_image(amber, tmp_path):
    """bin/amber --scene <obj> --device-build: the switch reaches create (AMBER_DEBUG_BVH prints another tree) and the image is the one without it."""
    from test_output_stage import parse_exr
    exe = Path(amber.library_path()).parent.parent / "bin" / "amber"
    obj = str(WL.room_mesh(3).write(tmp_path))
    outs, trees = [], []
    for extra in ([], ["--device-build"]):
        out = str(tmp_path / ("cli" + str(len(outs))))
        r = subprocess.run([str(exe), "--algorithm", "pt", "--scene", obj, "--width", "96", "--height", "64", "--spp", "16", "--seed", "5", "--samples-per-launch", "16",
                            "--output", out] + extra, capture_output=True, text=True, timeout=300, env=dict(os.environ, AMBER_DEBUG_BVH="1"))
        assert r.returncode == 0, r.stderr
        outs.append(parse_exr(out + ".exr"))
        trees.append([l for l in r.stderr.splitlines() if "scheduler" in l])
    assert len(trees[0]) == 1 and len(trees[1]) == 1 and trees[0] != trees[1], trees
    assert outs[0].any() and np.array_equal(bits(outs[0]), bits(outs[1]))
    usage = subprocess.run([str(exe), "--help"], capture_output=True, text=True, timeout=60)
    assert "--device-build" in usage.stderr + usage.stdout


# ---- 6: determinism ------------------------------------------------------------------------------------------------------------------------
def test_two_device_builds_of_the_terrain_are_byte_identical(amber, terrain):
    dumps = []
    for _ in range(2):
        pt = _tracer(amber, terrain[0], True)
        assert pt.build_info()["where"] == amber.BUILD_DEVICE
        dumps.append(pt.bvh_dump())
        pt.close()
    for key in ("nodes", "prims", "gmin", "step", "reach"):
        assert dumps[0][key].tobytes() == dumps[1][key].tobytes(), key
    assert dumps[0]["root"] == dumps[1]["root"] and dumps[0]["depth"] == dumps[1]["depth"]


# ---- 7: create is faster -------------------------------------------------------------------------------------------------------------------
def test_create_with_a_device_build_is_faster_than_with_the_host_build(amber, config3, terrain):
    """Median of 5 creates each, after a warm-up create of either kind (code objects loaded, allocator warm).  The host path is the parent commit's."""
    for name, hs in (("1M spheres", config3[0]), ("terrain", terrain[0])):
        med = {}
        for device in (False, True):
            _tracer(amber, hs, device).close()
            times, tree = [], []
            for _ in range(5):
                t0 = time.perf_counter()
                pt = _tracer(amber, hs, device)
                times.append((time.perf_counter() - t0) * 1e3)
                info = pt.build_info()
                pt.close()
                assert info["where"] == (amber.BUILD_DEVICE if device else amber.BUILD_HOST), (name, info)
                tree.append(info["tree_ms"])
            med[device] = (statistics.median(times), statistics.median(tree))
        print(f"\n{name}: create {med[False][0]:.1f} ms with the host build (tree stage {med[False][1]:.1f} ms), {med[True][0]:.1f} ms with the device build "
              f"(tree stage {med[True][1]:.1f} ms): {med[False][0] / med[True][0]:.1f}x")
        assert med[True][0] < med[False][0], (name, med)


# ---- 8: the product library ----------------------------------------------------------------------------------------------------------------
CHILD = r"""
import os, sys, json
sys.path.insert(0, {root!r})
import numpy as np
import amber_amd as A
from amber_amd import scenes
assert A.library_path().name == "libamber_hip.so" and not A.is_lab()
hs = A.HostScene.create_arrays(**scenes.random_spheres(60_000, 7))
pt = A.PathTracer(hs, A.Sensor.default(192, 108), seed=11, rows=(40, 56), flags=A.PT_FLAG_DEVICE_BUILD)
info = pt.build_info(); pt.render_pass(0, 16); img, rays = pt.download(); pt.close()
np.save(os.path.join({tmp!r}, "band.npy"), img)
print("RESULT " + json.dumps(dict(info=info, rays=int(rays))))
"""


def test_product_library_builds_on_the_device_and_renders_the_lab_builds_bits(amber, tmp_path):
    env = dict(os.environ, AMBER_AMD_LIB="libamber_hip.so")
    p = subprocess.run([sys.executable, "-c", CHILD.format(root=str(ROOT), tmp=str(tmp_path))], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    assert res["info"]["where"] == amber.BUILD_DEVICE and res["info"]["n_nodes"] > 10_000, res
    hs = amber.HostScene.create_arrays(**scenes.random_spheres(60_000, 7))
    pt = amber.PathTracer(hs, amber.Sensor.default(192, 108), seed=11, rows=(40, 56))          # the lab build, host tree
    pt.render_pass(0, 16)
    img, rays = pt.download()
    pt.close()
    assert rays == res["rays"] and np.array_equal(bits(np.load(tmp_path / "band.npy")), bits(img))

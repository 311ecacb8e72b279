"""Device-built, rebuilt and refitted trees of engine BVH are TIGHT, not only valid (tests/tree_reference.py has the argument and the validator).

The answer of engine BVH never depends on its tree, so no parity test can see a tree whose boxes are too large -- a refit that unions the new
boxes with the previous scene's, a stale word in the bottom-up hand-over, a padding applied twice, a plane word stepped outward three values
instead of one.  The only symptom would be lost speed.  Here every plane of every dumped tree is held to the numpy reference box of its child:
host-built trees within ONE representable binary16 value (which shows the validator right), device-built, rebuilt and refitted ones within TWO;
a refit A -> B -> C -> A of a device-built tree returns the handle's first dump byte for byte; and area_before / area_after of every update are
the figure the dumps give.  The last test corrupts a valid dump in the three ways above and shows that the tightness validator rejects what
test_device_build.validate_tree accepts.

Scenes: the smallest that still cross workgroup and XCD boundaries in the bottom-up hand-over, and trees of one leaf, one node and two nodes.
"""
import numpy as np
import pytest

from amber_amd import scenes
from amber_amd import workloads as WL
from test_device_build import _mixed_scene, _objects, _planar_scene, validate_tree
from test_update_objects import moved
from tree_reference import K_DEVICE, K_HOST, RANK_MAX, plane_ranks, reference_area, step_half, tree_levels, tree_tightness, widened_object_boxes

pytestmark = pytest.mark.gpu

SCENES = ["spheres", "mixed", "planar", "terrain", "room", "cornell"] + [f"spheres_{k}" for k in range(2, 10)]


def host_scene(amber, name):
    """(HostScene, keywords of PathTracer that put it through engine BVH)"""
    if name == "spheres":
        return amber.HostScene.create_arrays(**scenes.random_spheres(20_000, 7)), {}          # 79 workgroups of leaves
    if name == "mixed":
        return amber.HostScene.create_arrays(**_mixed_scene()), {}                             # all four kinds, non-unit axes
    if name == "planar":
        return amber.HostScene.create_arrays(**_planar_scene()), {}                            # no z extent, at z = 1234.5
    if name == "terrain":
        return amber.HostScene.create_arrays(**WL.terrain_mesh(16, 56).arrays()), {}
    if name == "room":
        return amber.HostScene.create_arrays(**WL.room_mesh(3).arrays()), {}
    if name == "cornell":
        return amber.HostScene.cornell_box(), dict(engine=amber.ENGINE_BVH)
    k = int(name.split("_")[1])                                                                # the pinhole's aperture triangle + k spheres
    return amber.HostScene.create_arrays(**dict(scenes.random_spheres(k, 3), n_blades=0)), dict(engine=amber.ENGINE_BVH)


def moved_records(rec, blades, seed):
    """test_update_objects.moved on flattened records; the aperture blades stay where they are (an update may not move the lens)"""
    out = rec.copy()
    out["p"] = moved(dict(kinds=rec["kind"], params=rec["p"]), seed)["params"]
    out[blades] = rec[blades]
    return out


class Trees:
    """One scene: the host scene, the records of A, B = moved(A, 101), C = moved(A, 202), their widened boxes (computed once), handles"""
    def __init__(self, amber, name):
        self.amber, self.name = amber, name
        self.hs, self.kw = host_scene(amber, name)
        lens = self.hs.flatten()[2]
        a = _objects(self.hs)
        blades = np.arange(int(lens.first_blade_object), int(lens.first_blade_object) + int(lens.n_blades))
        self.rec = {"A": a, "B": moved_records(a, blades, 101), "C": moved_records(a, blades, 202)}
        self.boxes = {k: widened_object_boxes(r) for k, r in self.rec.items()}
        self.n = len(a)

    def tracer(self, device):
        a = self.amber
        pt = a.PathTracer(self.hs, a.Sensor.default(64, 64), flags=a.PT_FLAG_DEVICE_BUILD if device else 0, **self.kw)
        info = pt.build_info()
        assert info["where"] == (a.BUILD_DEVICE if device else a.BUILD_HOST) and info["fallback_reason"] == 0, (self.name, info)   # never HOST_FALLBACK here
        return pt

    def tight(self, dump, key, k, what):
        st = tree_tightness(dump, self.rec[key], k, label=f"{self.name}, {what}", boxes=self.boxes[key])
        assert st["planes"] == 12 * len(dump["nodes"])
        print(f"\n{self.name}, {what}: {len(dump['nodes'])} nodes, {st['planes']} planes, looseness {st['looseness']} (allowed {k}), allowance needed {st['needed_ulps']:.3g} ulps")
        assert st["looseness"] <= k
        return st

    def update(self, pt, before, key, mode, first=0, count=None, what=""):
        """One update of objects [first, first + count) to scene `key`'s records.  area_before / area_after are the figures of the dumps taken before
        and after, to 1e-6 relative: the reported value is one binary32 rounding of a binary64 sum.  Returns (dump after, info)."""
        rec = self.rec[key] if count is None else self.rec[key][first:first + count]
        info = pt.update_flat(first, rec, mode)
        assert info["mode_used"] == mode and info["fallback_reason"] == 0, (self.name, what, info)
        after = pt.bvh_dump()
        if mode == self.amber.UPDATE_REFIT:
            assert after["nodes"][:, 6:8].tobytes() == before["nodes"][:, 6:8].tobytes() and after["prims"].tobytes() == before["prims"].tobytes()
        for name, dump in (("area_before", before), ("area_after", after)):
            want = reference_area(dump)
            print(f"\n{self.name}, {what}: {name} {info[name]!r}, from the dump {want!r}")
            if len(dump["nodes"]) == 0:
                assert info[name] == 0.0 and want == 0.0, (self.name, what, name, info)       # one leaf
            else:
                assert want > 0.0 and abs(info[name] - want) <= 1e-6 * want, (self.name, what, name, info[name], want)
        return after, info


_cache = {}


@pytest.fixture
def T(amber, request):
    name = request.param
    if name not in _cache:
        _cache.clear()                                                      # one scene's records at a time
        _cache[name] = Trees(amber, name)
    return _cache[name]


every_scene = pytest.mark.parametrize("T", SCENES, indirect=True)


# ---- trees as create builds them ---------------------------------------------------------------------------------------------------------
@every_scene
def test_host_built_trees_are_within_one_value_of_the_reference(T):
    """shows the validator right: PlaneWord stores the tightest representable value (tests/cpp/plane_word_check.cpp)"""
    pt = T.tracer(False)
    dump = pt.bvh_dump()
    pt.close()
    validate_tree(dump, T.rec["A"], T.name)
    T.tight(dump, "A", K_HOST, "host tree")


@every_scene
def test_device_built_trees_are_within_two_values_of_the_reference(T):
    pt = T.tracer(True)
    dump = pt.bvh_dump()
    pt.close()
    validate_tree(dump, T.rec["A"], T.name)
    T.tight(dump, "A", K_DEVICE, "device tree")


# ---- refit ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["host_tree", "device_tree"])
@every_scene
def test_refits_stay_tight_and_a_round_trip_returns_the_first_tree(T, start):
    """REFIT A -> B -> C -> A.  A refit is a function of topology and scene alone: a union with the previous scene's boxes, or an arrival counter
    left from the update before, passes A -> A and fails here -- the tree under B and C would be looser than K = 2 allows, and the tree after the
    round trip would not be the first one."""
    amber = T.amber
    pt = T.tracer(start == "device_tree")
    first = dump = pt.bvh_dump()
    areas = []
    for key in ("B", "C", "A"):
        dump, info = T.update(pt, dump, key, amber.UPDATE_REFIT, what=f"{start}, REFIT -> {key}")
        T.tight(dump, key, K_DEVICE, f"{start}, REFIT -> {key}")
        areas.append(info)
    pt.close()
    assert first["prims"].tobytes() == dump["prims"].tobytes() and first["nodes"][:, 6:8].tobytes() == dump["nodes"][:, 6:8].tobytes()
    if start == "device_tree":
        for key in ("nodes", "prims", "gmin", "step", "reach"):
            assert dump[key].tobytes() == first[key].tobytes(), (T.name, key)
        assert dump["root"] == first["root"] and dump["depth"] == first["depth"]
        assert areas[2]["area_after"] == areas[0]["area_before"]
    if T.name == "spheres":
        assert areas[0]["area_after"] != areas[0]["area_before"]           # moving the objects changes the figure


# ---- rebuild -------------------------------------------------------------------------------------------------------------------------------
@every_scene
def test_rebuilds_stay_tight(T):
    amber = T.amber
    pt = T.tracer(False)
    dump = pt.bvh_dump()
    for key in ("B", "A"):
        dump, info = T.update(pt, dump, key, amber.UPDATE_REBUILD, what=f"REBUILD -> {key}")
        validate_tree(dump, T.rec[key], T.name)
        T.tight(dump, key, K_DEVICE, f"REBUILD -> {key}")
    pt.close()


# ---- a partial range -------------------------------------------------------------------------------------------------------------------------
@every_scene
def test_a_refit_of_a_partial_range_stays_tight(T):
    """objects [n / 3, n / 3 + n / 100) take scene C's records, the others stay A's"""
    amber = T.amber
    first, count = T.n // 3, max(1, T.n // 100)
    assert first > 0
    rec = T.rec["A"].copy()
    rec[first:first + count] = T.rec["C"][first:first + count]
    T.rec["partial"], T.boxes["partial"] = rec, widened_object_boxes(rec)
    pt = T.tracer(True)
    dump, _ = T.update(pt, pt.bvh_dump(), "partial", amber.UPDATE_REFIT, first=first, count=count, what="REFIT of a partial range")
    pt.close()
    validate_tree(dump, rec, T.name)
    T.tight(dump, "partial", K_DEVICE, "REFIT of a partial range")


# ---- the tests bite ----------------------------------------------------------------------------------------------------------------------------
def _with_words(dump, nodes):
    return dict(dump, nodes=nodes)


def corrupt_one_plane(dump, steps=3):
    """one max plane stored `steps` representable values further out"""
    nodes = dump["nodes"].copy()
    _, hi = plane_ranks(dump)
    # (a left box whose max x plane lies well inside the right box's: the parent's box of this node, which is the union of the two, still contains it)
    candidates = np.flatnonzero((hi[:, 0, 0] + 2 * steps < hi[:, 1, 0]) & (hi[:, 1, 0] < RANK_MAX))
    node = int(candidates[len(candidates) // 2])
    w = int(nodes[node, 0])
    nodes[node, 0] = (w & 0xffff) | (int(step_half(w >> 16, steps)) << 16)
    return _with_words(dump, nodes), node


def corrupt_inner_child(dump):
    """one inner child's six planes replaced by its parent's own box in the grandparent"""
    nodes = dump["nodes"].copy()
    child = nodes[:, 6:8].view(np.int32)
    for g_side in (0, 1):                                                   # the grandparent is the root
        p = int(child[0, g_side])
        if p < 0:
            continue
        for side in (0, 1):
            if child[p, side] >= 0:
                nodes[p, 3 * side:3 * side + 3] = nodes[0, 3 * g_side:3 * g_side + 3]
                return _with_words(dump, nodes), p
    raise AssertionError("the root has no inner grandchild")


def corrupt_stale_subtree(dump_b, dump_a, level=4):
    """the plane words of one subtree copied from the tree of the same topology dumped under the previous scene"""
    assert dump_a["nodes"][:, 6:8].tobytes() == dump_b["nodes"][:, 6:8].tobytes()
    nodes = dump_b["nodes"].copy()
    child = nodes[:, 6:8].view(np.int32)
    frontier, members = tree_levels(dump_b)[level][:1], []
    while len(frontier):
        members.append(frontier)
        kids = child[frontier].ravel()
        frontier = kids[kids >= 0].astype(np.int64)
    members = np.concatenate(members)
    assert len(members) > 50
    nodes[members, :6] = dump_a["nodes"][members, :6]
    return _with_words(dump_b, nodes), members


@pytest.mark.parametrize("T", ["spheres"], indirect=True)
def test_the_tightness_validator_rejects_what_validate_tree_accepts(T):
    amber = T.amber
    pt = T.tracer(True)
    dump_a = pt.bvh_dump()
    dump_b, _ = T.update(pt, dump_a, "B", amber.UPDATE_REFIT, what="REFIT -> B")
    pt.close()
    T.tight(dump_a, "A", K_DEVICE, "device tree")
    T.tight(dump_b, "B", K_DEVICE, "REFIT -> B")
    # 1: a plane three values further out -- valid, and the gap this file closes: validate_tree cannot see it
    bad, node = corrupt_one_plane(dump_a)
    validate_tree(bad, T.rec["A"], "one plane three values out")
    with pytest.raises(AssertionError, match=f"a box is too large: the max plane of axis 0 of node {node}, side 0"):
        tree_tightness(bad, T.rec["A"], K_DEVICE, boxes=T.boxes["A"])
    # 2: a child box as large as its parent's -- valid too
    bad, node = corrupt_inner_child(dump_a)
    validate_tree(bad, T.rec["A"], "a child with its parent's box")
    with pytest.raises(AssertionError, match="a box is too large"):
        tree_tightness(bad, T.rec["A"], K_DEVICE, boxes=T.boxes["A"])
    # 3: a subtree that kept the previous scene's words through a refit
    bad, members = corrupt_stale_subtree(dump_b, dump_a)
    with pytest.raises(AssertionError, match="a box is too large"):
        tree_tightness(bad, T.rec["B"], K_DEVICE, boxes=T.boxes["B"])

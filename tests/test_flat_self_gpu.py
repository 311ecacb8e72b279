"""The flat-self shortcut of the 32-object two-phase engine (csrc/hip/filter_build.h "Flat self", dev_shading.h PathShade, dev_two_phase.h) against engine
LIST, which scans every object with the exact tests and has no shortcut of any kind.

A bounce ray that leaves a marked (axis-flat) triangle drops its self candidate without the self trip's arithmetic.  That must change nothing: the
framebuffer bits and the ray count of engine TWO_PHASE -- scouting, and with AMBER_PT_FLAG_NO_SCOUT -- equal LIST's on every scene, at max_depth 0, 2
and 16, and in a pass split 0..7, 7..64 (same ray count as the whole pass, LIST's bits for the same two passes); on the Cornell box every path's signature (hit objects and hit distances) equals LIST's.

Scenes, 64 x 64 at 64 samples: the Cornell box (every program triangle marked); a room with a box rotated about y, so that marked and unmarked starts
share a wave; the same room tilted about two axes, where nothing is marked; the Cornell box moved 1e4 of its size from the origin; and the seeds of
test_gpu_parity.test_fuzz_regressions with at most 32 objects, as tests/test_scout_replay.py lists them."""
import numpy as np
import pytest

from fuzz_scenes import scene_for_seed

pytestmark = pytest.mark.gpu
F32 = np.float32
W = H = 64
SPP, SEED = 64, 11
FUZZ = ((5, 0, 0), (1037, 0, 0), (2, 0, 0), (16, 0, 0), (40, 0, 0), (31296, 0, 1), (209769, 1, 1), (308053, 1, 0))   # (seed, scaled, extreme): <= 32 objects


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _rot(axis, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    i, j = {"x": (1, 2), "y": (2, 0), "z": (0, 1)}[axis]
    m = np.eye(3)
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def _room(tilt=None):
    """Five walls, a ceiling light, a box turned by 30 degrees about y (its top and bottom stay axis-flat, its sides do not) and a mirror sphere: 25 objects.
    tilt: a rotation applied to every vertex and centre, after which no triangle lies in an axis plane."""
    c8 = np.array([(-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)], np.float64)
    tris = []                                                                     # (material, 3 x 3 vertices)
    for a, b, c, d, m in ((0, 1, 2, 3, 1), (0, 4, 5, 1, 1), (3, 2, 6, 7, 1), (0, 3, 7, 4, 2), (1, 5, 6, 2, 3)):       # back, floor, ceiling, left, right
        tris += [(m, c8[[a, b, c]]), (m, c8[[c, d, a]])]
    L = np.array([(-0.5, 0.99, -0.5), (0.5, 0.99, -0.5), (0.5, 0.99, 0.5), (-0.5, 0.99, 0.5)])
    tris += [(0, L[[0, 1, 2]]), (0, L[[2, 3, 0]])]
    box = (c8 * np.array([0.3, 0.45, 0.3])) @ _rot("y", 30.0).T + np.array([0.3, -0.55, 0.1])
    for a, b, c, d in ((0, 1, 2, 3), (4, 7, 6, 5), (0, 4, 5, 1), (3, 2, 6, 7), (0, 3, 7, 4), (1, 5, 6, 2)):
        tris += [(1, box[[a, b, c]]), (1, box[[c, d, a]])]
    centre, r = np.array([-0.5, -0.65, -0.2]), 0.35
    if tilt is not None:
        tris = [(m, v @ tilt.T) for m, v in tris]
        centre = centre @ tilt.T
    objects = [(0, m, [float(F32(x)) for x in v.reshape(-1)]) for m, v in tris] + [(1, 4, [*[float(F32(x)) for x in centre], r])]
    materials = [(4, (20.0, 15.0, 10.0), 0.0), (0, (0.75, 0.75, 0.75), 0.0), (0, (0.75, 0.25, 0.25), 0.0), (0, (0.25, 0.75, 0.25), 0.0), (2, (0.9, 0.9, 0.9), 0.0)]
    return dict(objects=objects, materials=materials, transform=[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 4, 0, 0, 0, 1], focal_length=0.05, focus_distance=4.0,
                radius=0.02, n_blades=6)


def _flat_axes(objects):
    """How many triangles of a scene description have both edges exactly zero on some axis, in binary32 as the host stores them."""
    n = 0
    for kind, _, p in objects:
        if kind == 0:
            v = np.array(p[:9], F32).reshape(3, 3)
            e1, e2 = v[1] - v[0], v[2] - v[0]
            n += bool(((e1 == 0) & (e2 == 0)).any())
    return n


def _moved_cornell(amber):
    """The Cornell box, read back from the host model, moved 1e4 of its size away from the origin (camera and all)."""
    from amber_amd import scenes
    k = scenes.cornell_plus(0)
    p = k["params"].astype(np.float64)
    tri = k["kinds"] == amber.api.PRIM_TRIANGLE
    size = float(np.ptp(p[tri, :9].reshape(-1, 3), axis=0).max())
    off = 1.0e4 * size * np.array([1.0, -0.7, 0.4])
    p[tri, :9] += np.tile(off, 3)
    p[~tri, :3] += off
    k["params"] = p.astype(F32)
    t = [float(x) for x in k["transform"]]
    for r in range(3):
        t[4 * r + 3] += float(off[r])
    k["transform"] = t
    return amber.HostScene.create_arrays(**k)


@pytest.fixture(scope="module")
def scenes(amber):
    room, tilted = _room(), _room(_rot("x", 10.0) @ _rot("z", 15.0))
    assert len(room["objects"]) + 6 <= 32
    assert _flat_axes(room["objects"]) == 12 + 4 and _flat_axes(tilted["objects"]) == 0        # walls, light, the box's top and bottom | nothing
    out = {"cornell": amber.HostScene.cornell_box(), "room": amber.HostScene.create(**room), "tilted": amber.HostScene.create(**tilted),
           "moved": _moved_cornell(amber)}
    for seed, scaled, extreme in FUZZ:
        sc, _ = scene_for_seed(seed, scaled=bool(scaled), extreme=bool(extreme))
        assert len(sc["objects"]) + max(1, sc["n_blades"]) <= 32
        out[f"fuzz{seed}"] = amber.HostScene.create(**sc)
    return out


NAMES = ["cornell", "room", "tilted", "moved"] + [f"fuzz{s}" for s, _, _ in FUZZ]


def _render(amber, hs, engine, passes, flags=0, **kw):
    pt = amber.PathTracer(hs, amber.Sensor.default(W, H), seed=SEED, engine=engine, flags=flags, **kw)
    for first, n in passes:
        pt.render_pass(first, n)
    img, rays = pt.download()
    pt.close()
    return bits(img).copy(), rays


@pytest.mark.parametrize("name", NAMES)
def test_two_phase_equals_list(amber, scenes, name):
    """Framebuffer bits and ray count: scout on and off, max_depth 0 / 2 / 16, and a pass split 0..7, 7..64 against the whole pass."""
    hs = scenes[name]
    whole = ((0, SPP),)
    for depth in (0, 2, 16):
        ref_bits, ref_rays = _render(amber, hs, amber.ENGINE_LIST, whole, max_depth=depth)
        assert ref_rays >= W * H * SPP
        for flags in (0, amber.api.PT_FLAG_NO_SCOUT):
            got_bits, got_rays = _render(amber, hs, amber.ENGINE_TWO_PHASE, whole, flags=flags, max_depth=depth)
            assert got_rays == ref_rays, (name, depth, flags, got_rays, ref_rays)
            assert np.array_equal(got_bits, ref_bits), (name, depth, flags, int((got_bits != ref_bits).sum()))
        if depth == 0:
            # The same samples in two passes trace the same paths: the ray count is the whole pass's.  The framebuffer sums chunks of AMBER_ACCUM_CHUNK = 8
            # samples counted from each pass's first sample (include/amber_hip.h), so a split at 7 moves the chunk boundaries and engine LIST's own split
            # bits differ from its whole-pass bits wherever a pixel holds measurements on both sides of a boundary (the room: measured, printed below).
            # What must hold is equality with LIST rendered in the same two passes -- and through it with the whole pass wherever LIST's own two agree.
            split = ((0, 7), (7, SPP - 7))
            list_bits, list_rays = _render(amber, hs, amber.ENGINE_LIST, split)
            assert list_rays == ref_rays
            print(f"\n{name}: engine LIST, split pass == whole pass in {int((list_bits == ref_bits).all(axis=2).sum())} of {W * H} pixels")
            for flags in (0, amber.api.PT_FLAG_NO_SCOUT):
                got_bits, got_rays = _render(amber, hs, amber.ENGINE_TWO_PHASE, split, flags=flags)
                assert got_rays == ref_rays, (name, "split", flags, got_rays, ref_rays)
                assert np.array_equal(got_bits, list_bits), (name, "split", flags, int((got_bits != list_bits).sum()))
                same_in_list = (list_bits == ref_bits).all(axis=2)
                assert np.array_equal(got_bits[same_in_list], ref_bits[same_in_list]), (name, "split against the whole pass", flags)


def test_cornell_path_signatures_equal_list(amber, scenes):
    """Every path's hit-object sequence and hit distances, from the render kernels' signature instantiation and from the per-thread lab kernel."""
    hs, sn = scenes["cornell"], amber.Sensor.default(W, H)
    lst = amber.PathTracer(hs, sn, seed=SEED, engine=amber.ENGINE_LIST)
    two = amber.PathTracer(hs, sn, seed=SEED, engine=amber.ENGINE_TWO_PHASE)
    ref = lst.render_signatures(0, SPP)
    assert np.array_equal(two.render_signatures(0, SPP), ref)
    assert np.array_equal(two.kat_signatures(0, SPP), ref)
    assert len(np.unique(ref)) > W * H                                   # the paths differ: the comparison is not one of constants
    lst.close(); two.close()

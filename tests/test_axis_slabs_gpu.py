"""Axis slabs of the Phase-A filter (dev_two_phase.h: PhaseA) on the device.
 * Masks: amber_hip_kat_phase_a with the axis loops equals the same call with the general slab loop, bit for bit, on 2^16 rays per scene: rays of the
   model, rays with zero, subnormal, infinite and NaN components, rays nearly parallel to the slabs (|n.d| below 1e-6 and below AMBER_GRAZING) and
   origins outside the model box.  The reduced form only leaves out fma terms whose coefficient is an exact zero, and a ray that is not of the model
   keeps every candidate in both forms.
 * Images: engine TWO_PHASE and engine LIST give equal images and ray counts at 64 x 64, 64 spp.
Scenes: the Cornell box; cornell_plus(8) and cornell_plus(24) (33 and 49 objects: the grouped engine); a room with a rotated box (axis slabs and other
slabs together); a tilted room (no axis slab).  tests/cpp/axis_slabs_check.hip checks on the host what the builder classes."""
import numpy as np
import pytest

from amber_amd import api, scenes

N_RAYS = 1 << 16


def _rot(v, m):
    return (np.asarray(v, np.float32) @ np.asarray(m, np.float32).T).astype(np.float32)


def _quads_scene(amber, quads, quad_material, sphere=None):
    """create_arrays keywords for quads (a, b, c, d) of two triangles each, materials as mesh_room's, the lens of the other synthetic scenes."""
    tris, mat = [], []
    for (a, b, c, d), m in zip(quads, quad_material):
        tris += [np.concatenate([a, b, c]), np.concatenate([a, c, d])]; mat += [m, m]
    n = len(tris) + (1 if sphere is not None else 0)
    params, kinds = np.zeros((n, 12), np.float32), np.full(n, api.PRIM_TRIANGLE, np.uint32)
    params[: len(tris), :9] = np.array(tris, np.float32)
    if sphere is not None:
        params[-1, :4] = sphere; kinds[-1] = api.PRIM_SPHERE; mat.append(1)
    materials = [(api.MAT_DIFFUSE_LIGHT, (20.0, 20.0, 20.0), 0.0), (api.MAT_LAMBERTIAN, (0.75, 0.75, 0.75), 0.0), (api.MAT_LAMBERTIAN, (0.75, 0.25, 0.25), 0.0),
                 (api.MAT_LAMBERTIAN, (0.25, 0.75, 0.25), 0.0)]
    return dict(kinds=kinds, material_index=np.array(mat, np.uint32), params=params, materials=materials,
                transform=[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 4, 0, 0, 0, 1], focal_length=0.05, focus_distance=4.0, radius=0.01, n_blades=6)


def _box_quads(centre, half, rot):
    c8 = np.array([(-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)], np.float32) * np.asarray(half, np.float32)
    c8 = _rot(c8, rot) + np.asarray(centre, np.float32)
    return [tuple(c8[i] for i in q) for q in ((0, 1, 2, 3), (4, 7, 6, 5), (0, 4, 5, 1), (3, 2, 6, 7), (0, 3, 7, 4), (1, 5, 6, 2))]


def _room(amber, tilt):
    """Five walls of [-1, 1]^3 (open towards the camera) and a ceiling light, all turned by `tilt`; tilt = identity: with a box in it that is turned
    about y by the angle of the 3-4-5 triangle around the room's axis (its corners are mirror images in binary32, so its opposite sides are stored
    with equal normals and form slabs that are not axis slabs); else with a sphere."""
    eye = np.eye(3, dtype=np.float32)
    walls = _box_quads((0, 0, 0), (1, 1, 1), eye)
    quads = [walls[0], walls[2], walls[3], walls[4], walls[5]]                   # back, floor, ceiling, left, right
    material = [1, 1, 1, 2, 3]
    L = np.array([(-0.3, 0.99, -0.3), (0.3, 0.99, -0.3), (0.3, 0.99, 0.3), (-0.3, 0.99, 0.3)], np.float32)
    quads.append(tuple(L)); material.append(0)
    if tilt is None:
        quads += _box_quads((0, -0.6, 0), (0.25, 0.4, 0.25), [[0.8, 0, 0.6], [0, 1, 0], [-0.6, 0, 0.8]]); material += [1] * 6
        return _quads_scene(amber, quads, material)
    quads = [tuple(_rot(np.array(q), tilt)) for q in quads]
    return _quads_scene(amber, quads, material, sphere=(0.1, -0.5, 0.0, 0.3))


def _tilt():
    a, b = np.deg2rad(30.0), np.deg2rad(20.0)
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return (rx @ ry).astype(np.float32)


SCENES = ["cornell", "cornell_plus_8", "cornell_plus_24", "room_rotated_box", "tilted_room"]
_scene_cache = {}


def _scene(amber, name):
    if name not in _scene_cache:
        if name == "cornell":
            hs = amber.HostScene.cornell_box()
        elif name.startswith("cornell_plus_"):
            hs = amber.HostScene.create_arrays(**scenes.cornell_plus(int(name.rsplit("_", 1)[1])))
        else:
            hs = amber.HostScene.create_arrays(**_room(amber, None if name == "room_rotated_box" else _tilt()))
        _scene_cache[name] = hs
    return _scene_cache[name]


def _bounds(hs):
    """Centre and half extent (max norm) of the flattened scene's objects: where the filter's model box lies (scene_prep.h)."""
    objs, _, _ = hs.flatten()
    arr = np.frombuffer(objs, dtype=np.dtype([("kind", np.uint32), ("material", np.uint32), ("p", np.float32, (12,))]))
    tri = arr[arr["kind"] == 0]["p"][:, :9].reshape(-1, 3)
    sph = arr[arr["kind"] == 1]["p"]
    pts = np.concatenate([tri, sph[:, :3] - sph[:, 3:4], sph[:, :3] + sph[:, 3:4]])
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    return 0.5 * (lo + hi), 0.5 * (hi - lo).max()


def _rays(centre, half, seed):
    """2^16 rays: half of them rays of the model, the others with a special component, nearly parallel to an axis plane, or from outside."""
    rng = np.random.default_rng(seed)
    n = N_RAYS
    o = (centre + half * rng.uniform(-1.0, 1.0, (n, 3))).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 1e-45, -1e-45, np.inf, -np.inf, np.nan, 1e-7, -1e-7, 5e-7, -5e-7, 9.9e-7, 1.01e-6, 1e-5, -1e-5, 5e-4, -5e-4,
                        9.9e-4, 1.01e-3, -1.01e-3], np.float32)
    k = np.arange(n)
    comp, val = k % 3, special[(k // 3) % len(special)]
    in_d = (k >= n // 2) & (k < n * 3 // 4)                       # a special component of the direction (also |n.d| below 1e-6 and below AMBER_GRAZING for the axis planes)
    d[in_d, comp[in_d]] = val[in_d]
    two = in_d & (k % 5 == 0)                                      # ... two of them
    d[two, (comp[two] + 1) % 3] = special[(k[two] // 7) % len(special)]
    in_o = (k >= n * 3 // 4) & (k < n * 13 // 16)                  # a special component of the origin
    o[in_o, comp[in_o]] = val[in_o]
    out = (k >= n * 13 // 16) & (k < n * 15 // 16)                 # origins up to three model boxes away (the model box is twice the objects' box)
    o[out] = (centre + half * rng.uniform(-6.0, 6.0, (int(out.sum()), 3))).astype(np.float32)
    long_ = k >= n * 15 // 16                                      # |d| > 2
    d[long_] *= np.float32(2.5)
    return o, d


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_phase_a_masks_axis_loops_equal_general_loop(amber, name):
    hs = _scene(amber, name)
    centre, half = _bounds(hs)
    o, d = _rays(centre, half, SCENES.index(name) + 1)
    pt = amber.PathTracer(hs, amber.Sensor(64, 64, np.float32(0.036), np.float32(0.036)), seed=7, engine=amber.ENGINE_TWO_PHASE)
    try:
        on, off = pt.kat_phase_a(o, d, True), pt.kat_phase_a(o, d, False)
    finally:
        pt.close()
    n_objects = len(hs.flatten()[0])
    assert on.shape == off.shape == (N_RAYS, (n_objects + 31) // 32)
    differ = np.flatnonzero((on != off).any(axis=1))
    print(f"{name}: {n_objects} objects, {on.shape[1]} group(s), {len(differ)} of {N_RAYS} rays differ; "
          f"mean candidates per ray {np.unpackbits(off.view(np.uint8), axis=1).sum(axis=1).mean():.2f}")
    assert len(differ) == 0, [(int(i), o[i].tolist(), d[i].tolist(), [hex(x) for x in on[i]], [hex(x) for x in off[i]]) for i in differ[:5]]
    # the filter does filter: rays of the model keep fewer candidates than there are objects, rays that are not of the model keep all
    full = np.array([min(32, n_objects - 32 * g) for g in range(on.shape[1])])
    count = np.unpackbits(off.view(np.uint8).reshape(N_RAYS, -1, 4), axis=2).sum(axis=2)
    assert (count[: N_RAYS // 2].sum(axis=1) < n_objects).mean() > 0.9
    assert (count[N_RAYS * 15 // 16:] == full).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_two_phase_image_equals_list(amber, name):
    hs = _scene(amber, name)
    sensor = amber.Sensor(64, 64, np.float32(0.036), np.float32(0.036))
    out = {}
    for engine in (amber.ENGINE_TWO_PHASE, amber.ENGINE_LIST):
        pt = amber.PathTracer(hs, sensor, seed=11, engine=engine)
        try:
            pt.render_pass(0, 64)
            out[engine] = pt.download()
        finally:
            pt.close()
    (img_a, rays_a), (img_b, rays_b) = out[amber.ENGINE_TWO_PHASE], out[amber.ENGINE_LIST]
    print(f"{name}: rays {rays_a} / {rays_b}, mean {img_a.mean():.6g}")
    assert rays_a == rays_b and rays_a > 64 * 64 * 64
    assert np.array_equal(img_a.view(np.uint32), img_b.view(np.uint32))
    assert np.isfinite(img_a).all() and img_a.max() > 0

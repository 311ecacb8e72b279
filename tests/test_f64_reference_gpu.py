"""The kernels on the inputs of test_f64_reference_cpu.py: (a) within the recorded bounds of the binary64 reference, (b) bit for bit the oracle.
kat_cast / kat_sample / kat_eye / kat_light_ray / kat_lens_response / kat_radiance of the lab build, and amber_hip_pt_cast_rays through every product engine."""
import numpy as np
import pytest

import f64_inputs as I
import f64_reference as R
import oracle_binding as O
from test_f64_reference_cpu import (BOUNDS, CAMS, LIGHT_IDS, LIGHT_SETS, MIXED_CAP, RANDOM_CAP, check_eye, check_intersections, check_light, check_light_table,
                                    check_materials, check_response, check_round_trip, judged)

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def engines(amber):
    return [("LIST", amber.ENGINE_LIST, 0), ("TWO_PHASE", amber.ENGINE_TWO_PHASE, 0), ("BVH", amber.ENGINE_BVH, 0),
            ("BVH device tree", amber.ENGINE_BVH, amber.PT_FLAG_DEVICE_BUILD), ("BVH items", amber.ENGINE_BVH, amber.PT_FLAG_BVH_ITEMS),
            ("REFERENCE_BVH", amber.ENGINE_REFERENCE_BVH, 0)]


def same_bits(got, want, name):
    assert np.array_equal(got[0], want[0]), name
    hit = want[0] >= 0
    for k in (1, 2, 3):
        assert np.array_equal(bits(got[k][hit]), bits(want[k][hit])), (name, k)


def through_every_engine(amber, name, scene, o, d, aimed, cap, geometric=True):
    hs, osc = amber.HostScene.create(**scene), O.Scene.create(**scene, accel=O.ACCEL_BVH_CONS)
    osc.set_accel(O.ACCEL_LIST)
    want = I.oracle_casts(osc, o, d)
    sn = amber.Sensor.default(16, 16)
    pt = amber.PathTracer(hs, sn)
    got = pt.kat_cast(o, d)                                              # the lab build's known-answer kernel, engine AUTO
    pt.close()
    same_bits(got, want, name + " kat_cast")
    if geometric:
        check_intersections(name, scene, o, d, aimed, got, cap)          # (a): every engine below with these bits is within the bounds with them
    for label, eng, flags in engines(amber):
        pt = amber.PathTracer(hs, sn, engine=eng, flags=flags)
        got = pt.cast_rays(o, d)
        pt.close()
        if eng != amber.ENGINE_REFERENCE_BVH:
            same_bits(got, want, name + " " + label)
            continue
        osc.set_accel(O.ACCEL_BVH)                                       # the reference's own BVH: its ties and lost grazing hits are its own
        bvh = I.oracle_casts(osc, o, d)
        osc.set_accel(O.ACCEL_LIST)
        same_bits(got, bvh, name + " " + label)
        differs = (bvh[0] != want[0]) | ((want[0] >= 0) & (bits(bvh[1]) != bits(want[1])))
        tie = differs & (bvh[0] >= 0) & (want[0] >= 0) & (bits(bvh[1]) == bits(want[1]))
        lost = differs & ~tie & (want[0] >= 0) & ((bvh[0] < 0) | (bvh[1] > want[1]))
        assert not (differs & ~tie & ~lost).any(), name                  # every difference from List is an exact tie or a hit the tree lost
        if geometric and tie.any():                                      # the rays it answers as List does are covered above; a tie is a hit of the
            j = judged(name, scene, o[tie], d[tie], tuple(a[tie] for a in got))[4]   # OTHER object at the same distance: binary64 must accept that one too
            assert j["accepted"].all() and j["t_ok"].all()


@pytest.mark.parametrize("kind", range(4), ids=R.KIND_NAMES)
def test_primitive_through_every_engine(amber, kind):
    for name, scene, o, d, aimed, geometric in I.primitive_sets(kind):
        through_every_engine(amber, R.KIND_NAMES[kind] + " / " + name, scene, o, d, aimed, RANDOM_CAP, geometric)


def test_mixed_scene_through_every_engine(amber):
    scene, o, d, aimed = I.mixed_set()
    through_every_engine(amber, "mixed", scene, o, d, aimed, MIXED_CAP)


@pytest.mark.parametrize("name", [s[0] for s in I.MATERIAL_SETS])
def test_material_kernel_against_binary64(amber, name):
    kind, mats, importance, mat, nrm, do, state = I.material_items(name)
    hs = amber.HostScene.create(objects=[(R.SPHERE, m, [0.5 * m - 2.5, 0.0, 0.0, 0.2]) for m in range(len(I.MATERIALS))], materials=I.MATERIALS, **I.CAMERAS["thin6"])
    pt = amber.PathTracer(hs, amber.Sensor.default(16, 16))
    _, flat, _ = hs.flatten()                                             # the handle's own material table: find every material of the set in it
    key = lambda kind, rho, param: (kind, tuple(np.array(rho, np.float32).view(np.uint32)), np.float32(param).view(np.uint32))
    where = {key(f.kind, f.rho[:], f.param if f.kind in (R.PHONG, R.REFRACTION) else 0.0): i for i, f in enumerate(flat)}
    table = {m: where[key(*I.MATERIALS[m])] for m in mats}
    di, w, st = pt.kat_sample(np.array([table[int(m)] for m in mat], np.uint32), nrm, do, state, importance=importance)
    pt.close()
    odi, ow, used = I.oracle_materials(name)
    assert np.array_equal(bits(di), bits(odi)) and np.array_equal(bits(w), bits(ow))
    ref_state = state.copy()
    for k in range(int(used.max())):                                     # the kernel consumed as many draws as the oracle
        s = ref_state[used > k]
        R.xorshift_uniform(s)
        ref_state[used > k] = s
    assert np.array_equal(st, ref_state)
    check_materials(name, di, w, used)


@pytest.mark.parametrize("cam,W,H", CAMS, ids=[f"{c}-{w}x{h}" for c, w, h in CAMS])
def test_eye_ray_kernel_lands_in_its_pixel(amber, cam, W, H):
    scene = I.camera_scene(cam)
    hs, osc = amber.HostScene.create(**scene), O.Scene.create(**scene)
    px, sm = I.eye_items(W, H)
    pt = amber.PathTracer(hs, amber.Sensor.default(W, H), seed=I.EYE_SEED)
    eye = pt.kat_eye(px, sm)
    pt.close()
    assert np.array_equal(bits(eye), bits(I.oracle_eye(osc, W, H)))
    check_eye(osc, cam, W, H, eye)


# ------------------------------------------------------------------------------------------------------------------
# light tracing: the start of a light path, the lens response, Radiance()
# ------------------------------------------------------------------------------------------------------------------
def kernel_light(amber, hs, pt, states):
    """kat_light_ray with the table position mapped to the scene object: (origin, dir, weight, object, draws used), and the states after."""
    o, d, w, light, after = pt.kat_light_ray(states)
    table_object = np.array([f.object for f in hs.lights()], np.int64)
    assert (light < len(table_object)).all()
    return (o, d, w, table_object[light], I.draws_between(states, after)), after


def same_light_bits(got, after, osc, states):
    oo, od, ow, oobj, oafter = osc.light_rays(states, math=O.MATH_DEVICE)
    assert np.array_equal(got[3], oobj)
    assert np.array_equal(bits(got[0]), bits(oo)) and np.array_equal(bits(got[1]), bits(od)) and np.array_equal(bits(got[2]), bits(ow))
    assert np.array_equal(after, oafter)


@pytest.mark.parametrize("i", LIGHT_SETS, ids=LIGHT_IDS)
def test_light_ray_kernel_against_binary64(amber, i):
    name, scene, states, aimed, fam = I.light_sets()[i]
    hs, osc = amber.HostScene.create(**scene), O.Scene.create(**scene)
    check_light_table(scene, osc.lights(), hs.lights())
    pt = amber.PathTracer(hs, amber.Sensor.default(16, 16))
    got, after = kernel_light(amber, hs, pt, states)
    same_light_bits(got, after, osc, states)
    check_light(name, scene, states, aimed, fam, got)
    if name == "triangle / base":                                        # the launch's wave and block boundaries
        for n in I.SMALL_N:
            few, few_after = kernel_light(amber, hs, pt, states[:n])
            assert len(few[0]) == n and all(np.array_equal(bits(a), bits(b[:n])) for a, b in zip(few[:3], got[:3]))
            assert np.array_equal(few[3], got[3][:n]) and np.array_equal(few_after, after[:n])
    pt.close()


def test_light_ray_kernel_refuses_a_scene_without_lights(amber):
    hs = amber.HostScene.create(**I.camera_scene("thin6"))
    pt = amber.PathTracer(hs, amber.Sensor.default(16, 16))
    with pytest.raises(amber.AmberError, match="has no lights"):
        pt.kat_light_ray(np.ones(4, np.uint64))
    pt.close()


@pytest.mark.parametrize("cam,W,H", CAMS, ids=[f"{c}-{w}x{h}" for c, w, h in CAMS])
def test_lens_response_kernel_against_binary64(amber, cam, W, H):
    scene = I.camera_scene(cam)
    hs, osc = amber.HostScene.create(**scene), O.Scene.create(**scene)
    pos, do, aimed, fam, boundary, outside = I.response_items(cam, W, H)
    pt = amber.PathTracer(hs, amber.Sensor.default(W, H))
    got = pt.kat_lens_response(pos, do)
    pt.close()
    want = osc.lens_responses(W, H, pos, do, math=O.MATH_DEVICE)
    keep = ~outside                                                      # the pinhole's local z = 0: no parity asked (check_response holds them to the contract)
    assert np.array_equal(got[0][keep], want[0][keep]) and np.array_equal(got[1][keep], want[1][keep]) and np.array_equal(bits(got[2][keep]), bits(want[2][keep]))
    check_response(osc, cam, W, H, got)


@pytest.mark.parametrize("cam,W,H", CAMS, ids=[f"{c}-{w}x{h}" for c, w, h in CAMS])
def test_eye_rays_come_back_through_the_lens(amber, cam, W, H):
    scene = I.camera_scene(cam)
    hs, osc = amber.HostScene.create(**scene), O.Scene.create(**scene)
    px, sm = I.eye_items(W, H)
    pt = amber.PathTracer(hs, amber.Sensor.default(W, H), seed=I.EYE_SEED)
    eye = pt.kat_eye(px, sm)
    got = pt.kat_lens_response(eye[:, :3], eye[:, 3:6])
    pt.close()
    want = osc.lens_responses(W, H, eye[:, :3], eye[:, 3:6], math=O.MATH_DEVICE)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(bits(got[2]), bits(want[2]))
    check_round_trip(osc, cam, W, H, eye, got)


def test_radiance_kernel(amber, oracle):
    """Radiance() of every material of I.MATERIALS and of a second emitter: the oracle's bits, and zero exactly where the binary64 dot product
    of dir_out and the normal is <= 0 (outside the margin of the dot product's own rounding: three products and two sums of values <= 1,
    2.5 ulp of 1, taken 4 x and 4 x again as everywhere here)."""
    import ctypes as C
    materials = I.MATERIALS[:-1] + [(4, (0.25, 0.0, 2.0), 0.0)]          # (the Eye material is the one every scene appends itself)
    hs = amber.HostScene.create(objects=[(R.SPHERE, m, [0.5 * m - 2.5, 0.0, 0.0, 0.2]) for m in range(len(materials))], materials=materials, **I.CAMERAS["thin6"])
    _, flat, _ = hs.flatten()
    rng = np.random.default_rng(77)
    n = 512 * len(flat)
    mat = (np.arange(n) % len(flat)).astype(np.uint32)
    nrm = R.unit(rng.normal(size=(n, 3)))
    do = R.unit(rng.normal(size=(n, 3)))
    tang = I._perp(rng, nrm)
    k = n // 2                                                           # the second half: dir_out . n at 0 and STEPS ulp of 1 either side
    do[k:] = R.unit(tang[k:] + nrm[k:] * (rng.choice(I.STEPS, n - k) * 2.0 ** -24)[:, None])
    axis = rng.integers(0, 3, n // 8)                                    # and exactly 0: axis normals, dir_out in the plane
    nrm[-len(axis):] = np.eye(3)[axis]
    do[-len(axis):] = np.eye(3)[(axis + 1) % 3] * 0.6 + np.eye(3)[(axis + 2) % 3] * 0.8
    nrm, do = nrm.astype(np.float32), do.astype(np.float32)
    pt = amber.PathTracer(hs, amber.Sensor.default(16, 16))
    got = pt.kat_radiance(mat, nrm, do)
    with pytest.raises(amber.AmberError, match="material index out of range"):
        pt.kat_radiance(np.array([len(flat)], np.uint32), nrm[:1], do[:1])
    pt.close()
    want = np.zeros((n, 3), np.float32)
    oms = [O.OMaterial(f.kind, (C.c_float * 3)(*f.rho[:]), f.param) for f in flat]
    for i in range(n):
        oracle.oracle_radiance(C.byref(oms[int(mat[i])]), nrm.ctypes.data_as(C.POINTER(C.c_float * 3))[i], do.ctypes.data_as(C.POINTER(C.c_float * 3))[i],
                               want.ctypes.data_as(C.POINTER(C.c_float * 3))[i])
    assert np.array_equal(bits(got), bits(want))
    kinds = np.array([f.kind for f in flat])[mat]
    rho = np.array([f.rho[:] for f in flat], np.float32)[mat]
    cos = R.dot(do.astype(np.float64), nrm.astype(np.float64))
    margin = R.MARGIN_FACTOR * R.BOUND_FACTOR * 2.5 * 2.0 ** -23
    emitter = kinds == R.DIFFUSE_LIGHT
    assert (emitter.sum() >= 1000) and not got[~emitter].any()
    sure = np.abs(cos) > margin
    assert np.array_equal(got[emitter & sure & (cos > 0)], rho[emitter & sure & (cos > 0)]) and not got[emitter & sure & (cos < 0)].any()
    assert not got[emitter & (cos == 0)].any() and (emitter & (cos == 0)).sum() >= 10                     # the exact zeros: "<= 0" gives nothing
    near = emitter & ~sure
    assert (near.sum() >= 100) and all((g == r).all() or not g.any() for g, r in zip(got[near], rho[near]))
    assert 0.3 <= (cos[emitter & (np.arange(n) >= k)] > 0).mean() <= 0.7


def test_light_paths_of_the_product_start_where_the_stage_test_says(amber):
    """The join: the light-tracing kernel seeds path i of pass s with XorShiftSeed(hash(seed + 0x6C74), i, s) and starts it with
    GenerateLightRay; the oracle's light tracer starts with the function oracle_light_rays exports.  From those states kat_light_ray gives the
    oracle's first ray bit for bit -- on the scene, the frame and the seed whose lt_trace records test_light_tracing compares with that tracer."""
    from test_lt_render_pass import LIGHTS
    W, H, seed, sample = 48, 36, 13, 2
    hs, osc = amber.HostScene.create(**LIGHTS), O.Scene.create(**LIGHTS)
    L = O.load()
    states = np.array([L.oracle_xorshift_seed(seed + 0x6C74, path, sample) for path in range(256)], np.uint64)
    pt = amber.PathTracer(hs, amber.Sensor.default(W, H), seed=seed)
    got, after = kernel_light(amber, hs, pt, states)
    same_light_bits(got, after, osc, states)
    assert len(np.unique(got[3])) == 4                                   # all four light kinds of the scene start paths
    pt.close()

"""The kernels on the inputs of test_f64_reference_cpu.py: (a) within the recorded bounds of the binary64 reference, (b) bit for bit the oracle.
kat_cast / kat_sample / kat_eye of the lab build, and amber_hip_pt_cast_rays through every product engine."""
import numpy as np
import pytest

import f64_inputs as I
import f64_reference as R
import oracle_binding as O
from test_f64_reference_cpu import CAMS, MIXED_CAP, RANDOM_CAP, check_eye, check_intersections, check_materials, judged

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

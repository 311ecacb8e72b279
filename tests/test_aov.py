"""The first-hit AOVs on the GPU (amber_amd/csrc/hip/aov.inc): amber_hip_pt_aov_pass / _aov_clear / _aov_download / amber_hip_pt_device_aov.

One AOV pixel is eight binary32 sums -- albedo r g b, depth, normal x y z, coverage -- over the first hits of the pixel's eye rays, added in sample
order.  Every comparison is on bits (uint32 views), never within a tolerance: against the oracle's eye ray + cast accumulated in numpy's binary32,
between the engines, against the product's own ray query fed with the lab's eye rays, between split and unsplit passes, between bands and the full
frame, and across live updates.
Shapes: the oracle cases 24 x 16 (more than one workgroup of 256 pixels, a partial last one); the engine cases 48 x 40; the ray-query cases 1 x 1
(a single lane), 3 x 5, 53 x 37 (odd, eight workgroups with a partial last one) and 257 x 3 (rows longer than a workgroup).
"""
import ctypes
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle_binding as O
from amber_amd import api, scenes
from fuzz_scenes import scene_for_seed

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
W, H, SEED, FIRST, COUNT = 24, 16, 13, 3, 9

# the mixed-primitive scene of test_light_tracing (tests/test_gpu_parity.py): disk, triangle, sphere, cylinder, a floor, open sky
MIXED = dict(
    materials=[(4, (30.0, 20.0, 10.0), 0.0), (0, (0.7, 0.6, 0.5), 0.0), (2, (0.8, 0.8, 0.8), 0.0), (3, (1.0, 1.0, 1.0), 1.5), (4, (5.0, 5.0, 9.0), 0.0)],
    objects=[
        (2, 0, [0.0, 1.5, 0.0, 0.0, -1.0, 0.0, 0.6]),                      # disk light
        (0, 4, [-1.0, 1.4, -1.0, -1.0, 1.4, 1.0, -0.5, 1.4, 0.0]),        # triangle light
        (1, 0, [1.2, 0.8, 0.0, 0.15]),                                     # sphere light
        (3, 4, [-1.4, -0.5, 0.5, 0.0, 1.0, 0.0, 0.1, 0.6]),               # cylinder light
        (0, 1, [-3, -1, -3, 3, -1, 3, 3, -1, -3]), (0, 1, [-3, -1, -3, -3, -1, 3, 3, -1, 3]),
        (1, 2, [0.7, -0.6, -0.3, 0.4]), (1, 3, [0.0, -0.5, 0.8, 0.45]),
    ],
    transform=[1, 0, 0, 0, 0, 1, 0, 0.2, 0, 0, 1, 2.6, 0, 0, 0, 1], focal_length=0.05, focus_distance=2.6, radius=0.45, n_blades=5,
)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def records(hs):
    return np.frombuffer(hs.flatten()[0], dtype=api._RECORD).copy()


def aov_of(amber, hs, sensor, first, count, seed=SEED, **kw):
    """the AOVs of a fresh handle after one pass"""
    pt = amber.PathTracer(hs, sensor, seed=seed, **kw)
    pt.aov_pass(first, count)
    out = pt.aov_download()
    pt.close()
    return out


# ---- 1: against the oracle ---------------------------------------------------------------------------------------------------------------
def oracle_aov(osc, w, h, seed, first, count):
    """the sequential definition on the CPU: the oracle's eye ray of (pixel, sample), the oracle's cast, binary32 additions in sample order"""
    mats, objs = osc.materials(), osc.objects()
    out = np.zeros((h, w, 8), F32)
    for py in range(h):
        for px in range(w):
            for s in range(first, first + count):
                _, _, eye = osc.trace(w, h, seed, px, py, s, max_bounces=1)
                idx, t, _, nrm = osc.cast(eye[:3], eye[3:6])
                if idx >= 0:
                    term = np.concatenate([mats[objs[idx][1]][1], [t], nrm, [1.0]]).astype(F32)
                    out[py, px] = out[py, px] + term
    return out


_expected = {}


def expected(name):
    """computed once per scene, shared, never written to"""
    if name not in _expected:
        osc = O.Scene.cornell(O.ACCEL_LIST) if name == "cornell" else O.Scene.create(**MIXED)
        _expected[name] = oracle_aov(osc, W, H, SEED, FIRST, COUNT)
        _expected[name].setflags(write=False)
    return _expected[name]


@pytest.mark.parametrize("name,engine", [("cornell", "AUTO"), ("mixed", "LIST"), ("mixed", "BVH")])
def test_against_the_oracle(amber, name, engine):
    want = expected(name)
    coverage = float(want[..., 7].sum())
    print(f"\n{name}: coverage {coverage} of {COUNT * W * H} eye rays")
    if name == "mixed":
        assert 0 < coverage < COUNT * W * H                                  # hits and misses both occur
    else:
        assert coverage > 0
    hs = amber.HostScene.cornell_box() if name == "cornell" else amber.HostScene.create(**MIXED)
    got = aov_of(amber, hs, amber.Sensor.default(W, H), FIRST, COUNT, engine=getattr(amber, "ENGINE_" + engine))
    assert got.shape == (H, W, 8) and got.dtype == F32
    bad = bits(got) != bits(want)
    assert not bad.any(), (name, engine, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


# ---- 2: every engine agrees ----------------------------------------------------------------------------------------------------------------
# Engine REFERENCE_BVH answers as the reference's own tree does: on an exact distance tie the first object its leaf scan meets wins, not the lower
# scene index, and it loses the hits the reference's traversal loses.  So it equals the other engines on every pixel none of whose eye rays is such a
# ray -- the oracle says which (its List and its BVH acceleration on the same rays; seeds 2 and 11 hold coplanar overlapping triangles, a handful of
# pixels) -- and on EVERY pixel it equals the sums the oracle forms with the reference's BVH.
def engine_scenes(amber):
    out = []
    for seed in (2, 11, 16, 40, 12):                 # the ordinary seeds of test_fuzz_regressions; 12: a scene whose lens is the pinhole
        sc, _ = scene_for_seed(seed)
        out.append((f"fuzz seed {seed}", amber.HostScene.create(**sc), O.Scene.create(**sc, accel=O.ACCEL_BVH), len(sc["objects"]) + max(1, sc["n_blades"]), sc["n_blades"] == 0))
    kw = scenes.random_spheres(200, 7)
    out.append(("200 spheres", amber.HostScene.create_arrays(**kw), O.Scene.create_arrays(**kw, accel=O.ACCEL_BVH), 206, False))
    return out


def tie_pixels(osc, w, h, seed, first, count):
    """(h, w) bool: the pixels with an eye ray on which the oracle's List and the reference's BVH disagree"""
    rays = np.array([osc.trace(w, h, seed, px, py, s, max_bounces=1)[2][:6] for py in range(h) for px in range(w) for s in range(first, first + count)], F32)
    il, tl = osc.cast_many(rays[:, :3], rays[:, 3:], O.ACCEL_LIST)
    ib, tb = osc.cast_many(rays[:, :3], rays[:, 3:], O.ACCEL_BVH)
    return ((il != ib) | ((il >= 0) & (bits(tl) != bits(tb)))).reshape(h, w, count).any(axis=2)


def test_every_engine_agrees(amber):
    w, h = 48, 40
    sensor = amber.Sensor.default(w, h)
    pinholes = 0
    for name, hs, osc, n_obj, pinhole in engine_scenes(amber):
        pinholes += pinhole
        ref = aov_of(amber, hs, sensor, 0, 4, engine=amber.ENGINE_LIST)
        assert ref[..., 7].sum() > 0, name
        cases = [("AUTO", amber.ENGINE_AUTO, 0), ("BVH", amber.ENGINE_BVH, 0), ("BVH device build", amber.ENGINE_BVH, amber.PT_FLAG_DEVICE_BUILD),
                 ("BVH items", amber.ENGINE_BVH, amber.PT_FLAG_BVH_ITEMS)]
        if n_obj <= 128:
            cases.append(("TWO_PHASE", amber.ENGINE_TWO_PHASE, 0))
        for what, engine, flags in cases:
            got = aov_of(amber, hs, sensor, 0, 4, engine=engine, flags=flags)
            bad = bits(got) != bits(ref)
            assert not bad.any(), (name, what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        if n_obj > 80:                               # AUTO picks BVH
            pt = amber.PathTracer(hs, sensor, engine=amber.ENGINE_AUTO)
            assert pt.build_info()["where"] != amber.BUILD_NONE, name
            pt.close()
        got = aov_of(amber, hs, sensor, 0, 4, engine=amber.ENGINE_REFERENCE_BVH)
        ties = tie_pixels(osc, w, h, SEED, 0, 4)
        print(f"\n{name}: {int(ties.sum())} of {w * h} pixels hold an eye ray the reference's tree answers differently")
        assert ties.mean() < 0.01, name
        assert np.array_equal(bits(got)[~ties], bits(ref)[~ties]), (name, "REFERENCE_BVH")
        assert np.array_equal(bits(got), bits(oracle_aov(osc, w, h, SEED, 0, 4))), (name, "REFERENCE_BVH against the oracle's BVH")
    assert pinholes >= 1


# ---- 3: equals the product's own ray query ----------------------------------------------------------------------------------------------------
def aov_from_ray_queries(pt, hs, w, h, first, count):
    """the lab's eye rays (kat_eye) through cast_rays, accumulated in numpy's binary32 in sample order"""
    objs, mats, _ = hs.flatten()
    rho = np.array([m.rho[:] for m in mats], F32)[np.array([o.material for o in objs])]          # per object
    pixel = np.arange(w * h, dtype=np.uint32)
    out = np.zeros((w * h, 8), F32)
    for s in range(first, first + count):
        eye = pt.kat_eye(pixel, np.full(w * h, s, np.uint32))
        obj, t, _, nrm = pt.cast_rays(eye[:, :3], eye[:, 3:6])
        hit = obj >= 0
        term = np.concatenate([rho[np.maximum(obj, 0)], t[:, None], nrm, np.ones((w * h, 1), F32)], 1).astype(F32)
        out[hit] = out[hit] + term[hit]
    return out.reshape(h, w, 8)


@pytest.mark.parametrize("w,h", [(1, 1), (3, 5), (53, 37), (257, 3)])
def test_equals_the_ray_query_of_the_eye_rays(amber, w, h):
    assert amber.is_lab()
    hs = amber.HostScene.cornell_box()
    for first, count in ((0, 1), (5, 17)):
        pt = amber.PathTracer(hs, amber.Sensor.default(w, h), seed=SEED)
        want = aov_from_ray_queries(pt, hs, w, h, first, count)
        pt.aov_pass(first, count)
        got = pt.aov_download()
        pt.close()
        assert want[..., 7].sum() > 0
        assert np.array_equal(bits(got), bits(want)), (w, h, first, count, int((bits(got) != bits(want)).sum()))


# ---- 4: splitting and order --------------------------------------------------------------------------------------------------------------------
def test_splitting_and_order(amber):
    hs, sensor = amber.HostScene.cornell_box(), amber.Sensor.default(40, 24)
    whole = aov_of(amber, hs, sensor, 0, 16)
    pt = amber.PathTracer(hs, sensor, seed=SEED)
    pt.aov_pass(0, 7); pt.aov_pass(7, 9)
    assert np.array_equal(bits(pt.aov_download()), bits(whole)) and whole[..., 7].max() == 16
    pt.clear()                                                               # amber_hip_pt_clear leaves the AOVs alone
    assert np.array_equal(bits(pt.aov_download()), bits(whole))
    pt.aov_clear()
    assert not bits(pt.aov_download()).any()                                 # +0 everywhere
    # a pass leaves the image, the ray count and the kernel time as they were
    pt.render_pass(0, 8)
    img, rays = pt.download()
    timed = pt.kernel_time()
    pt.aov_pass(0, 16)
    assert np.array_equal(bits(pt.aov_download()), bits(whole))
    img2, rays2 = pt.download()
    assert np.array_equal(bits(img), bits(img2)) and rays == rays2 and rays > 0 and pt.kernel_time() == timed and timed[0] >= 1
    # aov_clear leaves the framebuffer alone
    pt.aov_clear()
    assert np.array_equal(bits(pt.download()[0]), bits(img))
    pt.close()
    # a pass between two render passes
    two = amber.PathTracer(hs, sensor, seed=SEED)
    two.render_pass(0, 8); two.render_pass(8, 8)
    want, want_rays = two.download()
    two.close()
    mid = amber.PathTracer(hs, sensor, seed=SEED)
    mid.render_pass(0, 8); mid.aov_pass(0, 16); mid.render_pass(8, 8)
    got, got_rays = mid.download()
    assert np.array_equal(bits(got), bits(want)) and got_rays == want_rays
    assert np.array_equal(bits(mid.aov_download()), bits(whole))
    ptr, n = mid.device_aov()
    assert ptr and n == 40 * 24
    mid.close()


# ---- 5: bands and stripes ------------------------------------------------------------------------------------------------------------------------
def test_bands_and_stripes(amber):
    hs, sensor = amber.HostScene.cornell_box(), amber.Sensor.default(40, 33)
    full = aov_of(amber, hs, sensor, 2, 5)
    assert full[..., 7].sum() > 0
    for kw, n_rows in ((dict(rows=(5, 29)), 24), (dict(stripe=(2, 6)), 12)):          # rows 0 1, 6 7, .. 30 31: 2 of every 6 of 33 rows
        pt = amber.PathTracer(hs, sensor, seed=SEED, **kw)
        pt.aov_pass(2, 5)
        got = pt.aov_download()
        assert got.shape == (n_rows, 40, 8) and len(pt.row_index) == n_rows, kw
        assert np.array_equal(bits(got), bits(full[pt.row_index])), kw
        assert pt.device_aov()[1] == n_rows * 40
        pt.close()


# ---- 6: live updates -------------------------------------------------------------------------------------------------------------------------------
def test_live_updates(amber):
    kw = scenes.random_spheres(300, 7)
    kw["params"][0, :4] = [-0.6, 0.0, 1.6, 0.3]                              # a large sphere in front of the others, left of the view's centre
    hs_a = amber.HostScene.create_arrays(**kw)
    kw_b = dict(kw, params=kw["params"].copy())
    kw_b["params"][0, :4] = [0.6, 0.0, 1.6, 0.3]                             # ... moved across the view
    hs_b = amber.HostScene.create_arrays(**kw_b)
    hs_c = amber.HostScene.create_arrays(**dict(kw_b, transform=[1, 0, 0, 0.3, 0, 1, 0, -0.2, 0, 0, 1, 4.5, 0, 0, 0, 1], focus_distance=4.5))   # the camera moved
    sensor = amber.Sensor.default(48, 40)
    want = {k: aov_of(amber, hs, sensor, 0, 4, engine=amber.ENGINE_BVH) for k, hs in (("A", hs_a), ("B", hs_b), ("C", hs_c))}
    assert not np.array_equal(bits(want["A"]), bits(want["B"])) and not np.array_equal(bits(want["B"]), bits(want["C"]))
    rec_a, rec_b = records(hs_a), records(hs_b)
    moved = np.flatnonzero((rec_a["p"] != rec_b["p"]).any(axis=1))
    assert len(moved) == 1
    first = int(moved[0])
    pt = amber.PathTracer(hs_a, sensor, seed=SEED, engine=amber.ENGINE_BVH)
    pt.aov_pass(0, 4)
    assert pt.update_flat(first, rec_b[first:first + 1], amber.UPDATE_REFIT)["mode_used"] == amber.UPDATE_REFIT
    assert np.array_equal(bits(pt.aov_download()), bits(want["A"]))          # enqueued before the update, downloaded after it: the old scene
    pt.aov_clear(); pt.aov_pass(0, 4)
    assert np.array_equal(bits(pt.aov_download()), bits(want["B"]))
    pt.aov_clear(); pt.aov_pass(0, 4)
    pt.update_lens(hs_c, amber.UPDATE_REFIT)
    assert np.array_equal(bits(pt.aov_download()), bits(want["B"]))          # the old lens
    pt.aov_clear(); pt.aov_pass(0, 4)
    assert np.array_equal(bits(pt.aov_download()), bits(want["C"]))
    pt.close()


# ---- 7: errors -----------------------------------------------------------------------------------------------------------------------------------
def test_errors(amber):
    lib = amber.load_library()
    hs, sensor = amber.HostScene.cornell_box(), amber.Sensor.default(20, 6)
    fresh = amber.PathTracer(hs, sensor, seed=1)
    fresh.render_pass(0, 8)
    good, good_rays = fresh.download()
    fresh.close()
    pt = amber.PathTracer(hs, sensor, seed=1)
    buf = np.full(20 * 6 * 8 + 16, 7.5, F32)
    p, dptr, n = buf.ctypes.data, ctypes.c_void_p(), ctypes.c_uint64(99)
    EINVAL, OK = -1, 0
    assert lib.amber_hip_pt_aov_pass(None, 0, 1) == EINVAL
    assert lib.amber_hip_pt_aov_clear(None) == EINVAL
    assert lib.amber_hip_pt_aov_download(None, p) == EINVAL
    assert lib.amber_hip_pt_aov_download(pt._h, None) == EINVAL
    assert lib.amber_hip_pt_device_aov(None, ctypes.byref(dptr), ctypes.byref(n)) == EINVAL
    assert lib.amber_hip_pt_device_aov(pt._h, None, ctypes.byref(n)) == EINVAL
    assert b"amber_hip_pt_device_aov" in lib.amber_hip_last_error()
    assert lib.amber_hip_pt_aov_pass(pt._h, 0xffffffff, 1) == EINVAL         # first_sample + n_samples = 2^32
    assert lib.amber_hip_pt_aov_pass(pt._h, 0x80000000, 0x80000000) == EINVAL
    assert b"amber_hip_pt_aov_pass" in lib.amber_hip_last_error()
    assert (buf == 7.5).all() and n.value == 99
    assert lib.amber_hip_pt_aov_pass(pt._h, 0, 0) == OK                      # n_samples == 0
    assert lib.amber_hip_pt_aov_pass(pt._h, 0xffffffff, 0) == OK
    assert not bits(pt.aov_download()).any()                                 # nothing of the above added anything
    assert lib.amber_hip_pt_aov_pass(pt._h, 0xfffffffe, 1) == OK             # the last sample index a pass can name
    assert pt.aov_download()[..., 7].max() == 1
    assert lib.amber_hip_pt_device_aov(pt._h, ctypes.byref(dptr), None) == OK and dptr.value
    pt.render_pass(0, 8)
    img, rays = pt.download()
    assert np.array_equal(bits(img), bits(good)) and rays == good_rays       # the handle renders what a fresh one renders
    pt.close()
    empty = amber.PathTracer(hs, sensor, seed=1, rows=(5, 5))
    assert lib.amber_hip_pt_aov_pass(empty._h, 0, 4) == OK and lib.amber_hip_pt_aov_clear(empty._h) == OK
    assert lib.amber_hip_pt_aov_download(empty._h, p) == OK and (buf == 7.5).all()          # nothing written
    assert lib.amber_hip_pt_device_aov(empty._h, ctypes.byref(dptr), ctypes.byref(n)) == OK and n.value == 0
    assert empty.aov_download().shape == (0, 20, 8)
    empty.close()


# ---- 8: the product library --------------------------------------------------------------------------------------------------------------------
PRODUCT_CHILD = r"""
import os, sys, json
sys.path.insert(0, {root!r})
import numpy as np
import amber_amd as A
assert A.library_path().name == "libamber_hip.so" and not A.is_lab()
pt = A.PathTracer(A.HostScene.cornell_box(), A.Sensor.default({w}, {h}), seed={seed})
pt.aov_pass({first}, {count})
np.save(os.path.join({tmp!r}, "aov.npy"), pt.aov_download())
ptr, n = pt.device_aov()
pt.close()
print("RESULT " + json.dumps(dict(n_pixels=n, has_pointer=bool(ptr))))
"""


def test_product_library(amber, tmp_path):
    assert amber.is_lab()
    script = PRODUCT_CHILD.format(root=str(ROOT), tmp=str(tmp_path), w=W, h=H, seed=SEED, first=FIRST, count=COUNT)
    p = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=dict(os.environ, AMBER_AMD_LIB="libamber_hip.so"), timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    assert res == dict(n_pixels=W * H, has_pointer=True)
    lab = aov_of(amber, amber.HostScene.cornell_box(), amber.Sensor.default(W, H), FIRST, COUNT)
    got = np.load(tmp_path / "aov.npy")
    assert np.array_equal(bits(got), bits(lab)) and np.array_equal(bits(got), bits(expected("cornell")))

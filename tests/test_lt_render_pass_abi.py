"""amber_hip_lt_render_pass at the edges of its contract: every AMBER_EINVAL and every AMBER_OK-with-nothing-changed of include/amber_hip.h leaves the
framebuffer and the ray counter as they were; info may be NULL; stale lights refuse as amber_hip_lt_trace does; the product library exports the
function and not the lab hook."""
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from test_lt_render_pass import LIGHTS, SEED, bits

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EINVAL = -1


@pytest.fixture(scope="module")
def scene(amber):
    return amber.HostScene.create(**LIGHTS)


def filled(amber, scene, **kw):
    """A handle whose framebuffer and ray counter hold something, and what they hold."""
    pt = amber.PathTracer(scene, amber.Sensor.default(32, 24), seed=SEED, **kw)
    pt.render_pass(0, 4)
    img, rays = pt.download()
    assert rays > 0
    return pt, bits(img).copy(), rays


def unchanged(pt, img, rays):
    now, now_rays = pt.download()
    return now_rays == rays and np.array_equal(bits(now), img)


def call(amber, pt, first, n, info=True):
    """(status, info or None) of the C function itself."""
    lib = amber.load_library()
    out = amber.LtPassInfo(1, 2, 3, 4, 5, 6)
    rc = lib.amber_hip_lt_render_pass(pt._h if pt is not None else None, first, n, C.byref(out) if info else None)
    return rc, out


def test_the_header_and_its_python_mirror(amber):
    text = (ROOT / "include" / "amber_hip.h").read_text()
    assert "AMBER_EINVAL = -1," in text and "#define AMBER_LT_SPLAT_CAPACITY0 65536u" in text and "#define AMBER_HIP_ABI_VERSION 3" in text
    assert "int amber_hip_lt_render_pass(amber_hip_pt*, uint32_t first_sample, uint32_t n_samples, AmberLtPassInfo* info" in text
    assert C.sizeof(amber.LtPassInfo) == 32 and amber.LT_SPLAT_CAPACITY0 == 65536
    assert [n for n, _ in amber.LtPassInfo._fields_] == ["n_splats", "n_rays", "n_launches", "n_repeats", "longest_run", "pad"]


def test_refusals_change_nothing(amber, scene):
    rc, info = call(amber, None, 0, 4)
    assert rc == EINVAL and b"null handle" in amber.load_library().amber_hip_last_error()
    assert (info.n_splats, info.n_rays, info.n_launches, info.n_repeats, info.longest_run) == (0, 0, 0, 0, 0)   # zeroed first
    einval = rc
    pt, img, rays = filled(amber, scene)
    for first, n in ((0xffffffff, 1), (0xfffffff0, 16), (1, 0xffffffff)):          # first + n > 2^32 - 1
        assert call(amber, pt, first, n)[0] == einval and unchanged(pt, img, rays)
    assert call(amber, pt, 0xfffffffe, 0)[0] == 0 and unchanged(pt, img, rays)
    pt.close()
    # a band, an empty band, stripes
    for kw in (dict(rows=(0, 12)), dict(rows=(8, 24)), dict(rows=(5, 5)), dict(stripe=(4, 8))):
        pt = amber.PathTracer(scene, amber.Sensor.default(32, 24), seed=SEED, **kw)
        pt.render_pass(0, 4)
        img, rays = pt.download()
        assert call(amber, pt, 0, 4)[0] == einval and b"band" in amber.load_library().amber_hip_last_error()
        assert unchanged(pt, bits(img).copy(), rays)
        pt.close()
    # the lab engine WAVEFRONT
    if amber.is_lab():
        pt, img, rays = filled(amber, scene, engine=amber.ENGINE_WAVEFRONT)
        assert call(amber, pt, 0, 4)[0] == einval and unchanged(pt, img, rays)
        with pytest.raises(amber.AmberError):
            pt.lt_render_pass(0, 4)
        pt.close()


def test_nothing_to_do_is_ok_and_changes_nothing(amber, scene):
    pt, img, rays = filled(amber, scene)
    rc, info = call(amber, pt, 7, 0)
    assert rc == 0 and unchanged(pt, img, rays) and (info.n_splats, info.n_rays, info.n_launches, info.pad) == (0, 0, 0, 0)
    assert pt.kernel_time()[0] == 1                                                # render_pass's launch, nothing more
    pt.close()
    dark = dict(LIGHTS, materials=[(0, (0.5, 0.5, 0.5), 0.0) if m[0] == 4 else m for m in LIGHTS["materials"]])   # the same scene, no emitter
    hs = amber.HostScene.create(**dark)
    pt = amber.PathTracer(hs, amber.Sensor.default(32, 24), seed=SEED)
    pt.render_pass(0, 4)
    img, rays = pt.download()
    rc, info = call(amber, pt, 0, 64)
    assert rc == 0 and unchanged(pt, bits(img).copy(), rays) and info.n_launches == 0
    assert pt.lt_trace(0, 64)[1] == 0
    pt.close()


def test_info_may_be_null(amber, scene):
    a = amber.PathTracer(scene, amber.Sensor.default(32, 24), seed=SEED)
    b = amber.PathTracer(scene, amber.Sensor.default(32, 24), seed=SEED)
    assert call(amber, a, 0, 400, info=False)[0] == 0
    rc, info = call(amber, b, 0, 400)
    (ia, ra), (ib, rb) = a.download(), b.download()
    assert rc == 0 and ra == rb == info.n_rays > 0 and np.array_equal(bits(ia), bits(ib)) and info.n_splats > 0 and ia.any() and info.pad == 0
    a.close(); b.close()


def test_stale_lights_refuse_as_lt_trace_does(amber, scene):
    objs, _, lens = scene.flatten()
    rec = np.frombuffer(objs, dtype=amber.api._RECORD).copy()
    pt = amber.PathTracer(scene, amber.Sensor.default(32, 24), seed=SEED, engine=amber.ENGINE_BVH)
    assert pt.lt_render_pass(0, 8)["n_rays"] > 0
    light = lens.first_blade_object + lens.n_blades + 2                            # the sphere light
    assert rec["kind"][light] == 1
    rec["p"][light, 0] += np.float32(0.05)
    pt.update_flat(0, rec)
    img, rays = pt.download()
    with pytest.raises(amber.AmberError, match="lights are stale after amber_hip_pt_update_objects: re-create the handle"):
        pt.lt_trace(0, 8)
    with pytest.raises(amber.AmberError, match="lights are stale after amber_hip_pt_update_objects: re-create the handle"):
        pt.lt_render_pass(8, 8)
    assert unchanged(pt, bits(img).copy(), rays)
    pt.close()


def test_the_product_exports_the_function_and_not_the_hook(amber):
    """A child process that loads only libamber_hip.so."""
    lib = ROOT / "amber_amd" / "lib" / amber.api.PRODUCT_LIB
    code = ("import ctypes, json, sys; lib = ctypes.CDLL(sys.argv[1]); "
            "print(json.dumps({n: hasattr(lib, n) for n in ('amber_hip_lt_render_pass', 'amber_hip_lt_trace', 'amber_hip_kat_lt_accumulate', 'amber_hip_kat_lt_stage_ms', "
            "'amber_hip_kat_light_ray', 'amber_hip_kat_lens_response', 'amber_hip_kat_radiance', 'amber_host_kat_scene_lights')}))")
    out = subprocess.run([sys.executable, "-c", code, str(lib)], capture_output=True, text=True, check=True).stdout
    assert json.loads(out) == {"amber_hip_lt_render_pass": True, "amber_hip_lt_trace": True, "amber_hip_kat_lt_accumulate": False, "amber_hip_kat_lt_stage_ms": False,
                               "amber_hip_kat_light_ray": False, "amber_hip_kat_lens_response": False, "amber_hip_kat_radiance": False,
                               "amber_host_kat_scene_lights": False}
    assert "amber_hip_lt_render_pass" in amber.api.ABI_SYMBOLS and "amber_hip_kat_lt_accumulate" in amber.api.LAB_SYMBOLS
    assert {"amber_hip_kat_light_ray", "amber_hip_kat_lens_response", "amber_hip_kat_radiance", "amber_host_kat_scene_lights"} <= set(amber.api.LAB_SYMBOLS)


def test_the_hook_refuses_what_it_cannot_place(amber, scene):
    if not amber.is_lab():
        pytest.fail("the suite runs on the lab build")
    from lt_accumulate_reference import records
    pt, img, rays = filled(amber, scene)
    with pytest.raises(amber.AmberError, match="pixel index out of range"):
        pt.kat_lt_accumulate(records([0, 1], [0, 0], [1, 1], [5, 32 * 24], np.ones((2, 3), np.float32)))
    assert unchanged(pt, img, rays)
    pt.close()
    band = amber.PathTracer(scene, amber.Sensor.default(32, 24), seed=SEED, rows=(0, 12))
    with pytest.raises(amber.AmberError, match="band"):
        band.kat_lt_accumulate(records([0], [0], [1], [5], np.ones((1, 3), np.float32)))
    band.close()

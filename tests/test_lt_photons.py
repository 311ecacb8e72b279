"""amber_hip_lt_trace_photons on the GPU: the vertices of the light paths, compared on BYTES with tests/photon_reference.py's walker (the definition
restated from the oracle's exported stages; test_photon_reference_cpu.py pins it), with the product's own splats and ray queries, and with itself
under every way the contract says a call can be cut up -- masks, pass splits, path splits, host and device pointers, a buffer that has to grow.

The scene is photon_reference.SCENE (all six material kinds, all four primitive kinds) at 24 x 16 -- 384 light paths per pass: more than one
workgroup, a partial last one -- seed 13, sensor scale 16, passes [0, 16): 3950 vertices, the longest path has 25."""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle_binding as O
import photon_reference as P

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
W, H, SEED, PASSES = P.W, P.H, P.SEED, P.PASSES
N_PATHS = W * H
EINVAL, ENOMEM = -1, -4


def sensor_of(amber, width=W, height=H):
    return amber.Sensor(width, height, np.float32(0.036 * P.SCALE), np.float32(0.036 / width * height * P.SCALE))


def tracer(amber, hs, engine="ENGINE_AUTO", flags=0, sensor=None, **kw):
    f = 0
    for name in ([flags] if isinstance(flags, str) else flags or []):
        f |= getattr(amber, name)
    return amber.PathTracer(hs, sensor or sensor_of(amber), seed=SEED, engine=getattr(amber, engine), flags=f, **kw)


def key_of(rec):
    return np.lexsort((rec["bounce"], rec["path"], rec["sample"]))


def merged(*lists):
    rec = np.concatenate(lists)
    return rec[key_of(rec)]


class Shared:
    """The scene, the walker's list, and the product's ALL list of a handle on engine AUTO: computed once, left unchanged."""

    def __init__(self, amber):
        self.hs = amber.HostScene.create(**P.SCENE)
        self.walker, self.want = P.reference(0)
        pt = tracer(amber, self.hs)
        self.all, self.info = pt.lt_trace_photons(0, PASSES, amber.PHOTON_ALL)
        self.splats, self.lt_rays = pt.lt_trace(0, PASSES)
        pt.close()
        self.all.setflags(write=False)


_shared = {}


@pytest.fixture(scope="module")
def S(amber):
    if "s" not in _shared:
        _shared["s"] = Shared(amber)
    return _shared["s"]


def test_the_entry_point_exists(amber):
    assert hasattr(amber.load_library(), "amber_hip_lt_trace_photons") and hasattr(amber.PathTracer, "lt_trace_photons")


# ---- every engine ----------------------------------------------------------------------------------------------------------------------------------
ENGINES = [("auto", "ENGINE_AUTO", None), ("list", "ENGINE_LIST", None), ("two_phase", "ENGINE_TWO_PHASE", None), ("bvh", "ENGINE_BVH", None),
           ("bvh_items", "ENGINE_BVH", "PT_FLAG_BVH_ITEMS"), ("bvh_device_build", "ENGINE_BVH", "PT_FLAG_DEVICE_BUILD"),
           ("reference_bvh", "ENGINE_REFERENCE_BVH", None)]


@pytest.mark.parametrize("label,engine,flags", ENGINES, ids=[e[0] for e in ENGINES])
def test_all_vertices_equal_the_walker_on_every_engine(amber, S, label, engine, flags):
    pt = tracer(amber, S.hs, engine, flags)
    rec, info = pt.lt_trace_photons(0, PASSES, amber.PHOTON_ALL)
    rays = pt.lt_trace(0, PASSES)[1]
    pt.close()
    if label == "reference_bvh":                                             # the reference's tree decides ties: the walker on the oracle's own BVH
        walker, want = P.reference(0, O.ACCEL_BVH)
        assert info["n_rays"] == rays == walker.casts
    else:
        walker, want = S.walker, S.want
        assert info["n_rays"] == rays == walker.casts == S.lt_rays
    print(f"\n{label}: {len(rec)} vertices, {info}")
    assert info["n_photons"] == info["n_written"] == len(rec) == len(want) and info["n_repeats"] == 0 and info["n_launches"] >= 1
    assert rec.dtype == P.PHOTON and rec.tobytes() == want.tobytes()


# ---- links to what the product already does ----------------------------------------------------------------------------------------------------------
def test_eye_vertices_through_the_lens_are_lt_traces_splats(amber, S):
    assert amber.is_lab()
    pt = tracer(amber, S.hs)
    eye, _ = pt.lt_trace_photons(0, PASSES, amber.PHOTON_EYE)
    reached, pixel, value = pt.kat_lens_response(eye["pos"], eye["dir_out"])
    pt.close()
    add = (eye["weight"] * value[:, None]) / np.float32(N_PATHS)
    keep = reached != 0
    assert len(S.splats) == keep.sum() >= 20 and len(eye) > keep.sum()
    for name, got in (("path", eye["path"]), ("sample", eye["sample"]), ("bounce", eye["bounce"]), ("pixel", pixel)):
        assert np.array_equal(got[keep], S.splats[name]), name
    assert np.ascontiguousarray(add[keep], np.float32).tobytes() == np.ascontiguousarray(S.splats["rgb"]).tobytes()


def test_consecutive_vertices_are_what_cast_rays_answers(amber, S):
    rec = S.all
    nxt = np.flatnonzero((rec["sample"][1:] == rec["sample"][:-1]) & (rec["path"][1:] == rec["path"][:-1]) & (rec["bounce"][1:] == rec["bounce"][:-1] + 1))
    n_paths_with_vertices = len(np.unique(rec["sample"].astype(np.uint64) * np.uint64(N_PATHS) + rec["path"]))
    assert len(nxt) == len(rec) - n_paths_with_vertices > 0                  # every vertex but a path's first has a predecessor: no gaps in `bounce`
    pt = tracer(amber, S.hs)
    obj, t, pos, nrm = pt.cast_rays(rec["pos"][nxt], -rec["dir_out"][nxt + 1])
    pt.close()
    assert np.array_equal(obj, rec["object"][nxt + 1])
    assert pos.tobytes() == np.ascontiguousarray(rec["pos"][nxt + 1]).tobytes() and nrm.tobytes() == np.ascontiguousarray(rec["normal"][nxt + 1]).tobytes()


# ---- masks, order ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [1, 2, 4, 8, 9])
def test_a_mask_is_the_filtered_list(amber, S, mask):
    pt = tracer(amber, S.hs)
    rec, info = pt.lt_trace_photons(0, PASSES, mask)
    pt.close()
    want = S.walker.select(S.all, mask)
    assert 0 < len(want) < len(S.all) and info["n_photons"] == len(want) and info["n_rays"] == S.lt_rays
    assert rec.tobytes() == want.tobytes()


def test_the_order_is_strictly_ascending(S):
    rec = S.all
    key = (rec["sample"].astype(object) << 64) | (rec["path"].astype(object) << 32) | rec["bounce"].astype(object)
    assert all(a < b for a, b in zip(key[:-1], key[1:])) and len(rec) == 3950


# ---- splitting ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", [1, 8, 9])
def test_pass_splits(amber, S, at):
    pt = tracer(amber, S.hs)
    a, ia = pt.lt_trace_photons(0, at, amber.PHOTON_ALL)
    b, ib = pt.lt_trace_photons(at, PASSES - at, amber.PHOTON_ALL)
    pt.close()
    assert len(a) and len(b) and ia["n_rays"] + ib["n_rays"] == S.lt_rays
    assert a.tobytes() + b.tobytes() == S.all.tobytes()


@pytest.mark.parametrize("at", [63, 64, 65, 256])
def test_path_splits_merge_by_key(amber, S, at):
    pt = tracer(amber, S.hs)
    a, ia = pt.lt_trace_photons(0, PASSES, amber.PHOTON_ALL, paths=(0, at))
    b, ib = pt.lt_trace_photons(0, PASSES, amber.PHOTON_ALL, paths=(at, N_PATHS))
    pt.close()
    assert len(a) and len(b) and ia["n_rays"] + ib["n_rays"] == S.lt_rays
    assert a["path"].max() < at <= b["path"].min()
    assert merged(a, b).tobytes() == S.all.tobytes()


def test_one_path_and_no_path(amber, S):
    pt = tracer(amber, S.hs)
    busiest = int(np.bincount(S.all["path"]).argmax())
    one, info = pt.lt_trace_photons(0, PASSES, amber.PHOTON_ALL, paths=(busiest, busiest + 1))
    none, info0 = pt.lt_trace_photons(0, PASSES, amber.PHOTON_ALL, paths=(7, 7))
    pt.close()
    want = S.all[S.all["path"] == busiest]
    assert len(want) >= 16 and one.tobytes() == want.tobytes() and PASSES <= info["n_rays"]
    assert len(none) == 0 and info0 == dict(n_photons=0, n_written=0, n_rays=0, n_launches=0, n_repeats=0)


def test_a_banded_handle_gives_the_same_list(amber, S):
    pt = tracer(amber, S.hs, rows=(4, 9))
    rec, _ = pt.lt_trace_photons(0, PASSES, amber.PHOTON_ALL)
    pt.close()
    assert rec.tobytes() == S.all.tobytes()


# ---- pointers, capacities ----------------------------------------------------------------------------------------------------------------------------
TORCH_CHILD = r"""
import json, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np, torch
import amber_amd as A
import photon_reference as P
hs = A.HostScene.create(**P.SCENE)
pt = A.PathTracer(hs, A.Sensor(P.W, P.H, np.float32(0.036 * P.SCALE), np.float32(0.036 / P.W * P.H * P.SCALE)), seed=P.SEED)
host, info = pt.lt_trace_photons(0, P.PASSES, A.PHOTON_ALL)
out = torch.full((len(host) + 3, 16), 7.0, dtype=torch.float32, device="cuda")
got, dinfo = pt.lt_trace_photons(0, P.PASSES, A.PHOTON_ALL, out=out)
same = got.cpu().numpy().tobytes() == host.tobytes()
tail_untouched = bool((out[len(host):] == 7.0).all().item())
raw = torch.zeros((len(host), 16), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
n, rinfo = pt.lt_trace_photons(0, P.PASSES, A.PHOTON_ALL, out=(raw.data_ptr(), len(host)))
same_raw = n == len(host) and raw.cpu().numpy().tobytes() == host.tobytes()
try:
    pt.lt_trace_photons(0, P.PASSES, A.PHOTON_ALL, out=(raw.data_ptr() + 4, 1))
    misaligned = "accepted"
except A.AmberError as e:
    misaligned = [e.code, "16-byte aligned" in str(e)]
again, _ = pt.lt_trace_photons(0, P.PASSES, A.PHOTON_ALL)
print("RESULT " + json.dumps(dict(same=same, tail_untouched=tail_untouched, same_raw=same_raw, infos=[info, dinfo, rinfo], misaligned=misaligned,
                                  good_after=again.tobytes() == host.tobytes(), n=len(host))))
"""


def _child(script, env=None, timeout=600, **fmt):
    p = subprocess.run([sys.executable, "-c", script.format(root=str(ROOT), tests=str(ROOT / "tests"), **fmt)], capture_output=True, text=True, env=env, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][7:])


def test_host_and_device_pointers_give_the_same_bytes(amber, S):
    pt = tracer(amber, S.hs)
    out = np.zeros(len(S.all) + 5, amber.PHOTON_DTYPE)
    out["bounce"] = 0xdeadbeef
    got, info = pt.lt_trace_photons(0, PASSES, amber.PHOTON_ALL, out=out)
    pt.close()
    assert got.tobytes() == S.all.tobytes() and info["n_written"] == len(S.all) and (out["bounce"][len(S.all):] == 0xdeadbeef).all()   # records beyond n_written: untouched
    res = _child(TORCH_CHILD)
    print("\n" + json.dumps(res))
    assert res["same"] and res["tail_untouched"] and res["same_raw"] and res["n"] == len(S.all)
    assert res["infos"][0] == res["infos"][1] == res["infos"][2]
    assert res["misaligned"] == [EINVAL, True] and res["good_after"]


def test_counting_call_exact_capacity_and_one_short(amber, S):
    lib = amber.load_library()
    pt = tracer(amber, S.hs)
    info = amber.PhotonInfo(1, 2, 3, 4, 5)
    assert lib.amber_hip_lt_trace_photons(pt._h, 0, PASSES, 0, N_PATHS, amber.PHOTON_ALL, None, 0, C.byref(info), 0) == 0      # counting, device flavour
    assert (info.n_photons, info.n_written, info.n_rays) == (len(S.all), 0, S.lt_rays)
    assert lib.amber_hip_lt_trace_photons(pt._h, 0, PASSES, 0, N_PATHS, amber.PHOTON_ALL, None, 0, None, amber.PHOTONS_HOST) == 0  # info may be NULL
    exact = np.zeros(len(S.all), amber.PHOTON_DTYPE)
    got, i1 = pt.lt_trace_photons(0, PASSES, amber.PHOTON_ALL, out=exact)
    assert got.tobytes() == S.all.tobytes() and i1["n_written"] == i1["n_photons"] == len(S.all)
    short = np.zeros(len(S.all) - 1, amber.PHOTON_DTYPE)
    with pytest.raises(amber.AmberError, match="photon buffer too small") as e:
        pt.lt_trace_photons(0, PASSES, amber.PHOTON_ALL, out=short)
    assert e.value.code == ENOMEM and e.value.info["n_photons"] == len(S.all) and e.value.info["n_written"] == 0
    got, i2 = pt.lt_trace_photons(0, PASSES, amber.PHOTON_ALL, out=exact)           # the handle stays working
    assert got.tobytes() == S.all.tobytes() and i2 == i1
    pt.close()


# ---- the rest of the handle ----------------------------------------------------------------------------------------------------------------------------
def test_framebuffer_ray_counter_and_kernel_time_are_left_alone(amber, S):
    pt, fresh = tracer(amber, S.hs), tracer(amber, S.hs)
    pt.render_pass(0, 4)
    img, rays = pt.download()
    before = (img.tobytes(), rays, pt.kernel_time())
    rec, _ = pt.lt_trace_photons(0, PASSES, amber.PHOTON_ALL)
    img, rays = pt.download()
    assert rec.tobytes() == S.all.tobytes() and rays > 0 and (img.tobytes(), rays, pt.kernel_time()) == before
    pt.render_pass(4, 4)
    fresh.render_pass(0, 4); fresh.render_pass(4, 4)
    (a, ra), (b, rb) = pt.download(), fresh.download()
    assert a.tobytes() == b.tobytes() and ra == rb and a.any()
    pt.close(); fresh.close()


def test_max_depth_three(amber, S):
    walker, want = P.reference(3)
    pt = tracer(amber, S.hs, max_depth=3)
    rec, info = pt.lt_trace_photons(0, PASSES, amber.PHOTON_ALL)
    pt.close()
    assert rec["bounce"].max() == 3 and info["n_rays"] == walker.casts and len(want) < len(S.all)
    assert rec.tobytes() == want.tobytes()


def test_after_update_lens_the_new_blades_are_seen(amber, S):
    moved = dict(P.SCENE, transform=[1, 0, 0, 0.3, 0, 1, 0, 0.1, 0, 0, 1, 2.2, 0, 0, 0, 1])
    hs_b = amber.HostScene.create(**moved)
    fresh = tracer(amber, hs_b, "ENGINE_BVH")
    want, wi = fresh.lt_trace_photons(0, PASSES, amber.PHOTON_ALL)
    fresh.close()
    pt = tracer(amber, S.hs, "ENGINE_BVH")
    first, _ = pt.lt_trace_photons(0, PASSES, amber.PHOTON_ALL)
    pt.update_lens(hs_b, amber.UPDATE_REBUILD)
    got, gi = pt.lt_trace_photons(0, PASSES, amber.PHOTON_ALL)
    pt.close()
    assert first.tobytes() == S.all.tobytes() and want.tobytes() != S.all.tobytes()
    assert got.tobytes() == want.tobytes() and gi["n_rays"] == wi["n_rays"]


def test_a_launch_that_outgrows_the_staging_buffer_is_repeated(amber, S):
    w, h = 384, 288
    sensor = sensor_of(amber, w, h)
    pt = tracer(amber, S.hs, sensor=sensor)
    rec, info = pt.lt_trace_photons(0, 1, amber.PHOTON_ALL)                  # (the counting call does not grow anything: the filling call repeats)
    print(f"\n{w} x {h}, one pass: {info}")
    assert info["n_photons"] == len(rec) > amber.PHOTON_CAPACITY0 and info["n_repeats"] >= 1 and info["n_launches"] == 1 + info["n_repeats"]
    again, info2 = pt.lt_trace_photons(0, 1, amber.PHOTON_ALL)               # the handle keeps what it grew to
    assert info2["n_repeats"] == 0 and again.tobytes() == rec.tobytes() and info2["n_rays"] == info["n_rays"]
    pt.close()
    halves = tracer(amber, S.hs, sensor=sensor)
    a, ia = halves.lt_trace_photons(0, 1, amber.PHOTON_ALL, paths=(0, w * h // 2))
    b, ib = halves.lt_trace_photons(0, 1, amber.PHOTON_ALL, paths=(w * h // 2, w * h))
    halves.close()
    assert ia["n_repeats"] == 0 and ib["n_repeats"] == 0 and max(len(a), len(b)) <= amber.PHOTON_CAPACITY0
    assert merged(a, b).tobytes() == rec.tobytes() and ia["n_rays"] + ib["n_rays"] == info["n_rays"]
    walker = P.Walker(P.oracle_scene(), SEED)
    want = walker.run(0, 1, 0, 2000)
    assert len(want) > 1000 and rec[rec["path"] < 2000].tobytes() == want.tobytes()


# ---- product against lab -------------------------------------------------------------------------------------------------------------------------------
PRODUCT_CHILD = r"""
import os, sys, json
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np
import amber_amd as A
import photon_reference as P
assert A.library_path().name == "libamber_hip.so" and not A.is_lab()
hs = A.HostScene.create(**P.SCENE)
for name, engine, flags in (("auto", A.ENGINE_AUTO, 0), ("bvh", A.ENGINE_BVH, 0), ("items", A.ENGINE_BVH, A.PT_FLAG_BVH_ITEMS), ("list", A.ENGINE_LIST, 0)):
    pt = A.PathTracer(hs, A.Sensor(P.W, P.H, np.float32(0.036 * P.SCALE), np.float32(0.036 / P.W * P.H * P.SCALE)), seed=P.SEED, engine=engine, flags=flags)
    rec, info = pt.lt_trace_photons(0, P.PASSES, A.PHOTON_ALL)
    np.save(os.path.join({tmp!r}, name + ".npy"), rec)
    pt.close()
print("RESULT " + json.dumps(dict(ok=True)))
"""


def test_product_library_gives_the_lab_builds_bytes(amber, S, tmp_path):
    assert amber.is_lab()
    _child(PRODUCT_CHILD, env=dict(os.environ, AMBER_AMD_LIB="libamber_hip.so"), tmp=str(tmp_path))
    for name in ("auto", "bvh", "items", "list"):
        assert np.load(tmp_path / (name + ".npy")).tobytes() == S.all.tobytes(), name


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_next_call_intact(amber, S):
    lib = amber.load_library()
    pt = tracer(amber, S.hs)
    buf = np.zeros(len(S.all), amber.PHOTON_DTYPE)
    dev = pt.device_framebuffer()[0]                                          # some device address: a refused call does not look behind it

    def call(h, first, n, begin, end, surfaces, out, capacity, flags):
        info = amber.PhotonInfo(9, 9, 9, 9, 9)
        rc = lib.amber_hip_lt_trace_photons(h, first, n, begin, end, surfaces, out, capacity, C.byref(info), flags)
        assert (info.n_photons, info.n_written, info.n_rays, info.n_launches, info.n_repeats) == (0, 0, 0, 0, 0) or rc == 0       # zeroed first, whatever the answer
        return rc

    def good():
        got, info = pt.lt_trace_photons(0, PASSES, amber.PHOTON_ALL, out=buf)
        assert got.tobytes() == S.all.tobytes() and info["n_rays"] == S.lt_rays

    good()
    HOST, ALL, p, n = amber.PHOTONS_HOST, amber.PHOTON_ALL, buf.ctypes.data, len(buf)
    cases = {
        "null handle": (None, 0, PASSES, 0, N_PATHS, ALL, p, n, HOST),
        "sample index overflow": (pt._h, 0xffffffff, 2, 0, N_PATHS, ALL, p, n, HOST),
        "path_begin > path_end": (pt._h, 0, PASSES, 9, 8, ALL, p, n, HOST),
        "path_end > W*H": (pt._h, 0, PASSES, 0, N_PATHS + 1, ALL, p, n, HOST),
        "no surfaces": (pt._h, 0, PASSES, 0, N_PATHS, 0, p, n, HOST),
        "unknown surface bits": (pt._h, 0, PASSES, 0, N_PATHS, 16 | 1, p, n, HOST),
        "unknown flag bits": (pt._h, 0, PASSES, 0, N_PATHS, ALL, p, n, HOST | 2),
        "null out with a capacity": (pt._h, 0, PASSES, 0, N_PATHS, ALL, None, n, HOST),
        "misaligned device pointer": (pt._h, 0, PASSES, 0, N_PATHS, ALL, dev + 8, 1, 0),
    }
    for name, args in cases.items():
        before = buf.tobytes()
        assert call(*args) == EINVAL, name
        assert amber.load_library().amber_hip_last_error(), name
        assert buf.tobytes() == before, name
        good()
    # AMBER_OK with zero photons
    for args in ((pt._h, 5, 0, 0, N_PATHS, ALL, p, n, HOST), (pt._h, 0, PASSES, 11, 11, ALL, p, n, HOST)):
        assert call(*args) == 0
    good()
    pt.close()
    # the lab engine WAVEFRONT
    wf = tracer(amber, S.hs, "ENGINE_WAVEFRONT")
    with pytest.raises(amber.AmberError, match="light tracing runs on the work-queue kernel") as e:
        wf.lt_trace_photons(0, PASSES, ALL, out=buf)
    assert e.value.code == EINVAL
    wf.close()
    # stale lights
    objs, _, lens = S.hs.flatten()
    rec = np.frombuffer(objs, dtype=amber.api._RECORD).copy()
    st = tracer(amber, S.hs, "ENGINE_BVH")
    light = lens.first_blade_object + lens.n_blades + 2                       # the sphere light
    assert rec["kind"][light] == 1
    rec["p"][light, 0] += np.float32(0.05)
    st.update_flat(0, rec)
    with pytest.raises(amber.AmberError, match="lights are stale after amber_hip_pt_update_objects: re-create the handle") as e:
        st.lt_trace_photons(0, PASSES, ALL, out=buf)
    assert e.value.code == EINVAL
    st.close()
    pt = tracer(amber, S.hs)
    good()
    pt.close()


WIDE_CHILD = r"""
import sys, json
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import amber_amd as A
import numpy as np
import photon_reference as P
assert str(A.library_path()).endswith("libamber_hip_wide.so")
pt = A.PathTracer(A.HostScene.create(**P.SCENE), A.Sensor.default(P.W, P.H), seed=P.SEED, engine=A.ENGINE_BVH)
try:
    pt.lt_trace_photons(0, 2, A.PHOTON_ALL)
    res = "accepted"
except A.AmberError as e:
    res = [e.code, "AMBER_BVH_WIDE" in str(e)]
rays = pt.lt_trace(0, 2)[1]
print("RESULT " + json.dumps(dict(res=res, rays=rays)))
"""


def test_the_wide_measurement_build_refuses(amber):
    """(`make wide` is incremental: test_build_options.py has built the library by the time the suite gets here)"""
    subprocess.run(["make", "-C", str(ROOT / "amber_amd" / "csrc"), "wide"], check=True, capture_output=True, timeout=900)
    res = _child(WIDE_CHILD, env=dict(os.environ, AMBER_AMD_LIB="libamber_hip_wide.so"))
    assert res["res"] == [EINVAL, True] and res["rays"] > 0


def test_a_scene_without_lights(amber):
    dark = dict(P.SCENE, materials=[(0, (0.7, 0.6, 0.5), 0.0)], objects=[(k, 0, p) for k, _, p in P.SCENE["objects"]])
    pt = tracer(amber, amber.HostScene.create(**dark))
    rec, info = pt.lt_trace_photons(0, PASSES, amber.PHOTON_ALL)
    pt.close()
    assert len(rec) == 0 and info == dict(n_photons=0, n_written=0, n_rays=0, n_launches=0, n_repeats=0)

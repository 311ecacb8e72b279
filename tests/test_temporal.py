"""amber_hip_pt_temporal on the GPU (amber_amd/csrc/hip/temporal.inc): the per-pixel history of the band's mean image, reprojected through the previous
lens, validated against the previous guide records, blended, and filtered by amber_hip_pt_denoise's levels.

Every comparison of floats is exact equality of bits with tests/temporal_reference.py, the numpy restatement of the contract in include/amber_hip.h
(pinned on its own by tests/test_temporal_reference_cpu.py); the bytes are held to the host's amber.tonemap of those floats (skipped, as in
tests/test_denoise.py, in a portable-math measurement build).
The synthetic frames are uploaded into the framebuffer and the AOV buffer as tests/test_denoise.py does, at the level kernel's edge shapes 1 x 1, 1 x 40,
37 x 23, 67 x 35 and 130 x 9.  They show a plane two units in front of the camera: the depth is the distance along every pixel's chief ray, albedo
blocks and a normal edge are fixed to the plane, a fifth of the pixels are misses, and from the third frame on a block of pixels is an object that came
30 % nearer.  A sequence is four frames: an empty history, the unchanged lens, a pan of 0.37 pixel with the camera 0.45 pixel higher, and a pan of a
quarter of the width (at least 2.6 pixels), after which part of the band reprojects outside it.  The handles are engine BVH's: amber_hip_pt_update_lens
moves the camera of no other engine."""
import ctypes
import functools
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import temporal_reference as T

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
N = 4
DIST = 2.0
POS = (0.1, 0.2, 0.5)
K = dict(max_history=3, k_normal=4.0, k_albedo=100.0, k_depth=10.0, k_color=0.25)      # a cap of 3: the fourth frame of a still camera would reach it
SHAPES = [(1, 1), (1, 40), (37, 23), (67, 35), (130, 9)]
# (levels, format, mirror): the mean at levels 0, 1 and 3 (both parities of the ping-pong); at 0 and 3 the mirrored mean and the bytes
CONFIGS = [(0, 0, False), (1, 0, False), (3, 0, False), (0, 0, True), (3, 0, True)] + [(l, f, m) for l in (0, 3) for f in (1, 2) for m in (False, True)]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _hip():
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return hip


def upload(pt, fb, aov):
    fptr, n_floats = pt.device_framebuffer()
    aptr, n_pixels = pt.device_aov()
    pt.sync()
    assert n_floats == fb.size and n_pixels * 8 == aov.size
    hip = _hip()
    assert hip.hipMemcpy(fptr, fb.ctypes.data, fb.nbytes, 1) == 0 and hip.hipMemcpy(aptr, aov.ctypes.data, aov.nbytes, 1) == 0      # hipMemcpyHostToDevice


def _transform(angle, pos):
    c, s = float(np.cos(angle)), float(np.sin(angle))
    return [c, 0, s, pos[0], 0, 1, 0, pos[1], -s, 0, c, pos[2], 0, 0, 0, 1]


@functools.lru_cache(maxsize=None)
def small_scene(amber, angle, pos, pinhole):
    """a light and three spheres behind the plane of the synthetic frames; only the lens and its blades matter to these tests"""
    kinds = np.array([1, 1, 1, 1], np.uint32)
    params = np.zeros((4, 12), np.float32)
    params[:, :4] = [[0.0, 1.5, -2.0, 0.3], [-0.6, 0.0, -2.5, 0.4], [0.5, -0.2, -2.2, 0.3], [0.0, -0.5, -3.0, 0.5]]
    materials = [(amber.api.MAT_DIFFUSE_LIGHT, (6.0, 5.0, 4.0), 0.0), (amber.api.MAT_LAMBERTIAN, (0.7, 0.7, 0.7), 0.0)]
    return amber.HostScene.create_arrays(kinds=kinds, material_index=np.array([0, 1, 1, 1], np.uint32), params=params, materials=materials,
                                         transform=_transform(angle, pos), focal_length=0.02, focus_distance=1.5, radius=0.05, n_blades=0 if pinhole else 6)


class Sequence:
    """The four lenses, the four synthetic frames and the reference's states, infos and outputs of one shape -- computed once, left unchanged"""
    def __init__(self, amber, w, h, pinhole, rows):
        self.w, self.h, self.rows = w, h, rows or (0, h)
        self.sensor_rec = amber.Sensor.default(w, h)
        self.sensor = (w, h, F32(self.sensor_rec.scene_width), F32(self.sensor_rec.scene_height))
        sd = float(small_scene(amber, 0.0, POS, pinhole).flatten()[2].sensor_distance)
        pixel = float(np.arctan(float(self.sensor[2]) / w / sd))
        up = 0.45 * DIST * float(self.sensor[3]) / h / sd
        big = max(2.6, 0.25 * w)
        cams = [(0.0, POS), (0.0, POS), (0.37 * pixel, (POS[0], POS[1] + up, POS[2])), (min(0.6, float(np.arctan(big * float(self.sensor[2]) / w / sd))), (POS[0], POS[1] + up, POS[2]))]
        self.scenes = [small_scene(amber, a, p, pinhole) for a, p in cams]
        self.lenses = [T.lens_of(s.flatten()[2]) for s in self.scenes]
        assert self.lenses[0].words == self.lenses[1].words != self.lenses[2].words != self.lenses[3].words
        self.frames = [self.frame(i, sd) for i in range(4)]
        self.states, self.infos, state = [], [], T.empty_state(self.rows[1] - self.rows[0], w)
        for (fb, aov), L in zip(self.frames, self.lenses):
            state, info = T.accumulate(state, fb, aov, N, L, self.sensor, self.rows[0], K["max_history"], K["k_normal"], K["k_albedo"], K["k_depth"])
            self.states.append(state)
            self.infos.append(info)
        assert [i["moved"] for i in self.infos] == [False, False, True, True]

    def frame(self, index, sd):
        w, h, L = self.w, self.h, self.lenses[index]
        rng = np.random.default_rng(1000 * w + 10 * h + index)
        y, x = np.mgrid[self.rows[0]:self.rows[1], 0:w]
        s = np.stack([((x + 0.5) / w - 0.5) * float(self.sensor[2]), ((y + 0.5) / h - 0.5) * float(self.sensor[3]), np.full(x.shape, float(L.sensor_distance))], -1)
        g = -(s @ L.global_.astype(np.float64).reshape(3, 3).T)
        g = g / np.linalg.norm(g, axis=-1, keepdims=True)
        o = L.origin.astype(np.float64)
        t = (POS[2] - DIST - o[2]) / g[..., 2]                                  # binary64: the distance to the plane z = POS.z - DIST along the chief ray
        P = o + t[..., None] * g
        fx, fy = DIST * float(self.sensor[2]) / w / sd, DIST * float(self.sensor[3]) / h / sd      # a pixel's footprint on the plane
        clean = np.where((P[..., 0] < POS[0])[..., None], F32([0.8, 0.2, 0.1]), F32([0.1, 0.3, 0.9]))
        fb = ((clean + rng.normal(0.0, 0.3, x.shape + (3,))) * N).astype(F32)
        cov = rng.integers(0, 5, x.shape).astype(F32)
        albedo = np.array([0.7, 0.75, 0.2], F32)[(np.floor(P[..., 0] / (7 * fx)) + np.floor(P[..., 1] / (5 * fy))).astype(np.int64) % 3]
        normal = np.where((P[..., 0] < POS[0])[..., None], F32([0, 0, 1]), F32([0.6, 0, 0.8]))
        depth = t * (1 + 0.02 * rng.random(x.shape))
        rows = x.shape[0]
        if index >= 2:
            depth[rows // 3:rows // 2, w // 4:w // 2] *= 0.7                     # an object that came nearer
        depth = depth.astype(F32)
        if w * rows > 1:
            cov[0, min(w - 1, 3)], depth[0, min(w - 1, 3)] = 2, 0                # a pixel that was hit at depth 0
        else:
            cov[0, 0] = 3
        aov = np.zeros(x.shape + (8,), F32)
        aov[..., 0:3] = (albedo * cov)[..., None]
        aov[..., 3] = depth * cov
        aov[..., 4:7] = normal * cov[..., None]
        aov[..., 7] = cov
        return fb, aov

    @functools.lru_cache(maxsize=None)
    def output(self, index, levels):
        c = self.states[index]["hist"][..., 0:3].copy()
        a, n, z, rz = self.states[index]["guide"]
        with np.errstate(all="ignore"):
            kc = F32(K["k_color"])
            for i in range(levels):
                c = T.D.level(c, a, n, z, rz, F32(K["k_normal"]), F32(K["k_albedo"]), F32(K["k_depth"]), kc, 1 << i)
                kc = kc * F32(4)
        return c


@functools.lru_cache(maxsize=None)
def sequence(amber, w, h, pinhole=False, rows=None):
    return Sequence(amber, w, h, pinhole, rows)


def play(amber, pt, seq, levels, fmt, mirror, first):
    """the four frames on a handle whose lens is the first one and whose history is empty; everything is compared after every call"""
    glibc = amber.math_mode() == amber.MATH_GLIBC
    rows, w = seq.rows[1] - seq.rows[0], seq.w
    for i, ((fb, aov), scene) in enumerate(zip(seq.frames, seq.scenes)):
        if i >= 2 or (i == 0 and not first):
            pt.update_lens(scene)
        upload(pt, fb, aov)
        got = pt.temporal(N, levels=levels, format=fmt, mirror=mirror, **K)
        what = (w, seq.h, i, levels, fmt, mirror)
        hist = pt.history_download()
        assert hist.shape == (rows, w, 8) and hist.dtype == F32
        wrong = int((bits(hist) != bits(seq.states[i]["hist"])).any(axis=-1).sum())
        assert wrong == 0, (what, f"history: {wrong} of {rows * w} pixels differ")
        want = seq.output(i, levels)
        flip = (lambda a: a[:, ::-1]) if mirror else (lambda a: a)
        if fmt == amber.RESOLVE_MEAN_F32:
            assert got.dtype == F32 and got.shape == (rows, w, 3)
            wrong = int((bits(got) != bits(flip(want))).any(axis=-1).sum())
            assert wrong == 0, (what, f"mean: {wrong} of {rows * w} pixels differ")
        else:
            if not glibc:
                continue                                                        # (the history above was compared; only the bytes need glibc's powf)
            ldr = flip(amber.tonemap(want))
            assert got.dtype == np.uint8 and np.array_equal(got[..., :3], ldr), (what, "bytes")
            assert got.shape == (rows, w, 4 if fmt == amber.RESOLVE_RGBA8 else 3) and (fmt != amber.RESOLVE_RGBA8 or (got[..., 3] == 255).all()), what


def check_coverage(seq):
    """asserted on the reference's own output, so that the device test cannot pass vacuously"""
    s0, s1 = seq.states[0]["hist"], seq.states[1]["hist"]
    assert (s0[..., 3] == 1).all() and not seq.infos[0]["kept"].any()
    assert seq.infos[1]["kept"].any() and (s1[..., 3][seq.infos[1]["kept"]] == 2).all()
    if seq.w * seq.h > 40:
        for i in (2, 3):
            info = seq.infos[i]
            assert info["fractional"].mean() >= 0.1 and (~info["kept"]).mean() >= 0.1, (seq.w, seq.h, i, info["fractional"].mean(), (~info["kept"]).mean())
        assert (seq.states[2]["hist"][..., 3] == 3).any()                        # the cap of 3 was reached, and on frame 4 it acts
        assert seq.states[3]["hist"][..., 3].max() == 3 and ((seq.states[3]["hist"][..., 3] % 1) != 0).any()      # ... next to fractional lengths


# ---- 1: synthetic frames -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SHAPES)
def test_synthetic_frames(amber, w, h):
    seq = sequence(amber, w, h)
    check_coverage(seq)
    pt = amber.PathTracer(seq.scenes[0], seq.sensor_rec, seed=3, engine=amber.ENGINE_BVH)
    assert not pt.history_download().any()                                      # a history never used reads as zeros
    for j, (levels, fmt, mirror) in enumerate(CONFIGS):
        play(amber, pt, seq, levels, fmt, mirror, first=j == 0)
        pt.temporal_reset()
        assert not pt.history_download().any()                                  # ... and so does an emptied one
    pt.close()


def test_a_pinhole_and_a_band(amber):
    for pinhole, rows in ((True, None), (False, (5, 29))):
        seq = sequence(amber, 67, 35, pinhole, rows)
        assert int(seq.scenes[0].flatten()[2].kind) == (1 if pinhole else 0)
        check_coverage(seq)
        pt = amber.PathTracer(seq.scenes[0], seq.sensor_rec, seed=3, engine=amber.ENGINE_BVH, rows=rows)
        for j, (levels, fmt, mirror) in enumerate([(0, 0, False), (3, 0, True), (1, 2, False)]):
            play(amber, pt, seq, levels, fmt, mirror, first=j == 0)
            pt.temporal_reset()
        pt.close()
    whole, band = sequence(amber, 67, 35), sequence(amber, 67, 35, False, (5, 29))
    assert not np.array_equal(band.states[3]["hist"], whole.states[3]["hist"][5:29])      # the band reprojects within itself, with py the global row


def test_a_striped_handle_is_refused_and_an_empty_band_is_ok(amber):
    lib = amber.load_library()
    hs = amber.HostScene.cornell_box()
    striped = amber.PathTracer(hs, amber.Sensor.default(64, 48), seed=5, rows=(2, 24), stripe=(2, 6))
    striped.render_pass(0, 8)
    buf = np.full(8 * 64 * 3, 0xAB, np.uint8)
    params = amber.TemporalParams(levels=5, **{k: v for k, v in K.items()})
    assert lib.amber_hip_pt_temporal(striped._h, 8, ctypes.byref(params), amber.RESOLVE_RGB8, buf.ctypes.data, buf.nbytes, amber.RESOLVE_HOST) == -1      # AMBER_EINVAL
    assert b"amber_hip_pt_temporal" in lib.amber_hip_last_error() and b"strip" in lib.amber_hip_last_error() and (buf == 0xAB).all()
    with pytest.raises(amber.AmberError):
        striped.temporal(8)
    assert striped.resolve(8).shape == (8, 64, 3) and not striped.history_download().any()
    striped.close()
    empty = amber.PathTracer(hs, amber.Sensor.default(64, 48), seed=5, rows=(5, 5))
    for fmt in (0, 1, 2):
        assert lib.amber_hip_pt_temporal(empty._h, 8, ctypes.byref(params), fmt, None, 0, 0) == 0
        assert lib.amber_hip_pt_temporal(empty._h, 8, ctypes.byref(params), fmt, None, 0, amber.RESOLVE_HOST | amber.RESOLVE_MIRROR_X) == 0
    assert empty.temporal(8).shape == (0, 64, 3) and empty.history_download().shape == (0, 64, 8) and empty.device_history() == (None, 0)
    empty.temporal_reset()
    assert lib.amber_hip_pt_temporal(empty._h, 8, ctypes.byref(params), amber.RESOLVE_RGB8, None, 3, 0) == -1
    empty.close()


# ---- 2: rendered frames ------------------------------------------------------------------------------------------------------------------------
def moved(amber, hs, shift):
    """the scene's lens `shift` further, with its blade records: the explicit pair amber_hip_pt_update_lens takes"""
    objs, _, lens = hs.flatten()
    rec = np.frombuffer(objs, dtype=amber.api._RECORD)
    blades = rec[lens.first_blade_object:lens.first_blade_object + lens.n_blades].copy()
    blades["p"][:, :9] = (blades["p"][:, :9].reshape(-1, 3, 3) + F32(shift)).reshape(-1, 9)
    new = type(lens).from_buffer_copy(lens)
    for i in range(3):
        new.origin[i] = float(F32(lens.origin[i]) + F32(shift[i]))
    return lens, new, blades, rec


@pytest.mark.parametrize("light_traced", [False, True], ids=["render_pass", "lt_render_pass"])
def test_rendered_frames(amber, light_traced):
    hs, sensor = amber.HostScene.cornell_box(), amber.Sensor.default(64, 48)
    lens_a, lens_b, blades_b, rec = moved(amber, hs, (0.06, 0.03, 0.0))           # about 1.4 and 0.7 pixels at the box's middle depth
    spp = 4 if light_traced else 64
    sens = (64, 48, F32(sensor.scene_width), F32(sensor.scene_height))
    pt = amber.PathTracer(hs, sensor, seed=5, engine=amber.ENGINE_BVH)

    def render(first):
        pt.clear()
        pt.aov_clear()
        (pt.lt_render_pass if light_traced else pt.render_pass)(first, spp)
        pt.aov_pass(first, spp)
        return pt.download()[0], pt.aov_download()

    kw = dict(levels=2, max_history=32, k_normal=4.0, k_albedo=100.0, k_depth=10.0, k_color=0.0)      # k_color = 0: the guides alone (tests/test_denoise.py says why)
    fb_a, aov_a = render(0)
    denoised = pt.denoise(spp, format=amber.RESOLVE_MEAN_F32)
    got_a = pt.temporal(spp, format=amber.RESOLVE_MEAN_F32, **kw)
    want_a, state, _ = T.temporal(T.empty_state(48, 64), fb_a, aov_a, spp, T.lens_of(lens_a), sens, **kw)
    assert np.array_equal(bits(got_a), bits(want_a)) and np.array_equal(bits(pt.history_download()), bits(state["hist"]))
    # what leaves the history alone: an update of objects (the same geometry again), a lens update, both clears
    hist = pt.history_download()
    other = np.delete(np.arange(len(rec)), np.arange(lens_a.first_blade_object, lens_a.first_blade_object + lens_a.n_blades))[:2]
    pt.update_flat(int(other[0]), rec[other[0]:other[0] + 1].copy())
    assert np.array_equal(bits(pt.history_download()), bits(hist))
    pt.update_lens((lens_b, blades_b))
    assert np.array_equal(bits(pt.history_download()), bits(hist))
    fb_b, aov_b = render(spp)
    assert np.array_equal(bits(pt.history_download()), bits(hist)) and hist[..., 3].min() == 1 == hist[..., 3].max()
    # what the call leaves alone: the sums, the AOVs, the ray count, the kernel time, denoise()'s bytes
    rays, time_before = pt.download()[1], pt.kernel_time()
    denoised_b = pt.denoise(spp, format=amber.RESOLVE_MEAN_F32)
    got_b = pt.temporal(spp, format=amber.RESOLVE_MEAN_F32, **kw)
    want_b, state_b, info = T.temporal(state, fb_b, aov_b, spp, T.lens_of(lens_b), sens, **kw)
    assert info["moved"] and info["kept"].mean() > 0.25 and (~info["kept"]).any() and info["fractional"].mean() > 0.25, (info["kept"].mean(), info["fractional"].mean())
    assert np.array_equal(bits(got_b), bits(want_b)) and np.array_equal(bits(pt.history_download()), bits(state_b["hist"]))
    after, rays_after = pt.download()
    assert np.array_equal(bits(after), bits(fb_b)) and rays_after == rays and rays > 0 and np.array_equal(bits(pt.aov_download()), bits(aov_b))
    assert pt.kernel_time() == time_before and time_before[0] >= 1
    assert np.array_equal(bits(pt.denoise(spp, format=amber.RESOLVE_MEAN_F32)), bits(denoised_b)) and denoised.shape == denoised_b.shape
    # the lens unchanged: a running mean of the same frame is the frame (h + (c - h) / N with c == h where nothing was reset)
    got_c = pt.temporal(spp, format=amber.RESOLVE_MEAN_F32, **kw)
    want_c, state_c, info_c = T.temporal(state_b, fb_b, aov_b, spp, T.lens_of(lens_b), sens, **kw)
    assert not info_c["moved"] and np.array_equal(bits(got_c), bits(want_c)) and np.array_equal(bits(pt.history_download()), bits(state_c["hist"]))
    # temporal_reset: the next call equals a first call
    pt.temporal_reset()
    assert not pt.history_download().any()
    got_d = pt.temporal(spp, format=amber.RESOLVE_MEAN_F32, **kw)
    want_d, state_d, _ = T.temporal(T.empty_state(48, 64), fb_b, aov_b, spp, T.lens_of(lens_b), sens, **kw)
    assert np.array_equal(bits(got_d), bits(want_d)) and np.array_equal(bits(pt.history_download()), bits(state_d["hist"])) and (state_d["hist"][..., 3] == 1).all()
    ptr, n_pixels = pt.device_history()
    assert ptr and n_pixels == 64 * 48
    back = np.zeros((48, 64, 8), F32)
    pt.sync()
    assert _hip().hipMemcpy(back.ctypes.data, ptr, back.nbytes, 2) == 0 and np.array_equal(bits(back), bits(state_d["hist"]))      # hipMemcpyDeviceToHost
    pt.close()


# ---- 3: stream order ---------------------------------------------------------------------------------------------------------------------------
TORCH_CHILD = r"""
import os, sys, json
sys.path.insert(0, {root!r})
import numpy as np
import torch
torch.cuda.init()
import amber_amd as A
dev = torch.device("cuda", 0)
W, H, SPP = 40, 24, 16
hs, sensor = A.HostScene.cornell_box(), A.Sensor.default(W, H)
kw = dict(levels=2, k_color=0.0, max_history=8)
ref = A.PathTracer(hs, sensor, seed=2)
want = []
for frame in range(2):
    ref.clear(); ref.aov_clear(); ref.render_pass(frame * SPP, SPP); ref.aov_pass(frame * SPP, SPP)
    want.append((ref.temporal(SPP, format=A.RESOLVE_RGBA8, **kw), ref.temporal(SPP, format=A.RESOLVE_MEAN_F32, mirror=True, **kw), ref.history_download()))
ref.close()
pt = A.PathTracer(hs, sensor, seed=2)
ext = torch.cuda.ExternalStream(pt.stream(), device=dev)
out = dict(bytes=[], mean=[], history=[])
with torch.cuda.stream(ext):
    for frame in range(2):
        rgba = torch.full((H, W, 4), 7, dtype=torch.uint8, device=dev)
        mean = torch.full((H, W, 3), 7, dtype=torch.float32, device=dev)
        pt.clear(); pt.aov_clear(); pt.render_pass(frame * SPP, SPP); pt.aov_pass(frame * SPP, SPP)       # nothing waits between the passes and the two calls
        returned = pt.temporal(SPP, format=A.RESOLVE_RGBA8, out=rgba, **kw)
        pt.temporal(SPP, format=A.RESOLVE_MEAN_F32, mirror=True, out=mean, **kw)
        pt.sync()
        out["bytes"].append(bool(returned is rgba and np.array_equal(rgba.cpu().numpy(), want[frame][0])))
        out["mean"].append(bool(np.array_equal(mean.cpu().numpy().view(np.uint32), want[frame][1].view(np.uint32))))
        out["history"].append(bool(np.array_equal(pt.history_download().view(np.uint32), want[frame][2].view(np.uint32))))
out["lengths"] = sorted(set(want[1][2][..., 3].reshape(-1).tolist()))
out["picture"] = int(len(np.unique(want[1][0])))
try:
    pt.temporal(SPP, format=A.RESOLVE_RGBA8, out=torch.empty((H, W, 3), dtype=torch.uint8, device=dev), **kw); out["refused"] = False
except A.AmberError:
    out["refused"] = True
pt.close()
print("RESULT " + json.dumps(out))
"""


def test_a_torch_tensor_on_the_handles_stream(amber):
    p = subprocess.run([sys.executable, "-c", TORCH_CHILD.format(root=str(ROOT))], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    assert res["bytes"] == [True, True] and res["mean"] == [True, True] and res["history"] == [True, True], res
    # two calls per frame: the still camera's history is four frames long (shorter where a pixel's coverage changed with the new samples)
    assert res["lengths"][-1] == 4.0 and set(res["lengths"]) <= {1.0, 2.0, 3.0, 4.0} and res["picture"] >= 2 and res["refused"], res


# ---- 4: errors ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_are_einval_and_leave_the_history_as_it_was(amber):
    lib = amber.load_library()
    pt = amber.PathTracer(amber.HostScene.cornell_box(), amber.Sensor.default(20, 6), seed=1)
    pt.render_pass(0, 8)
    pt.aov_pass(0, 8)
    pt.temporal(8, format=amber.RESOLVE_RGBA8)
    hist = pt.history_download()
    assert (hist[..., 3] == 1).all()
    fb, aov = pt.download()[0], pt.aov_download()
    lens = T.lens_of(amber.HostScene.cornell_box().flatten()[2])
    sens = (20, 6, F32(amber.Sensor.default(20, 6).scene_width), F32(amber.Sensor.default(20, 6).scene_height))
    _, state, _ = T.temporal(T.empty_state(6, 20), fb, aov, 8, lens, sens)
    assert np.array_equal(bits(hist), bits(state["hist"]))
    HOST = amber.RESOLVE_HOST
    buf = np.full(20 * 6 * 12 + 64, 0xAB, np.uint8)
    p = buf.ctypes.data

    def P(**over):
        f = dict(levels=5, max_history=32, k_normal=4.0, k_albedo=100.0, k_depth=10.0, k_color=0.25)
        reserved = over.pop("reserved", (0, 0))
        f.update(over)
        return ctypes.byref(amber.TemporalParams(reserved=(ctypes.c_uint32 * 2)(*reserved), **f))
    cases = {"null handle": (None, 8, P(), 1, p, 360, HOST), "null params": (pt._h, 8, None, 1, p, 360, HOST), "n_samples == 0": (pt._h, 0, P(), 1, p, 360, HOST),
             "levels 9": (pt._h, 8, P(levels=9), 1, p, 360, HOST), "max_history 0": (pt._h, 8, P(max_history=0), 1, p, 360, HOST),
             "max_history 65536": (pt._h, 8, P(max_history=65536), 1, p, 360, HOST), "reserved[0]": (pt._h, 8, P(reserved=(1, 0)), 1, p, 360, HOST),
             "reserved[1]": (pt._h, 8, P(reserved=(0, 1)), 1, p, 360, HOST),
             "unknown format": (pt._h, 8, P(), 3, p, 360, HOST), "unknown flag bits": (pt._h, 8, P(), 1, p, 360, HOST | 4),
             "null out": (pt._h, 8, P(), 1, None, 360, HOST), "null out, device": (pt._h, 8, P(), 1, None, 360, 0),
             "one byte short": (pt._h, 8, P(), 1, p, 359, HOST), "one byte long": (pt._h, 8, P(), 1, p, 361, HOST), "zero bytes": (pt._h, 8, P(), 1, p, 0, HOST)}
    for field in ("k_normal", "k_albedo", "k_depth", "k_color"):
        for bad in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
            cases[f"{field} = {bad}"] = (pt._h, 8, P(**{field: bad}), 1, p, 360, HOST)
    for what, args in cases.items():
        assert lib.amber_hip_pt_temporal(*args) == -1, what                               # AMBER_EINVAL
        assert b"amber_hip_pt_temporal" in lib.amber_hip_last_error(), what
        assert (buf == 0xAB).all(), what                                                   # no effect
        assert np.array_equal(bits(pt.history_download()), bits(hist)), what               # ... on the history either
        # and the handle works: a successful call with levels 0 and a cap of 1 takes the frame again and leaves the very history it found
        # (N = min(1 + 1, 1) = 1, alpha = 1: h + (c - h) * 1 with c == h)
        assert lib.amber_hip_pt_temporal(pt._h, 8, P(levels=0, max_history=1), 1, p, 360, HOST) == 0, what
        assert np.array_equal(bits(pt.history_download()), bits(hist)), what
        buf[:] = 0xAB
    assert lib.amber_hip_pt_temporal_reset(None) == -1 and lib.amber_hip_pt_history_download(pt._h, None) == -1 and lib.amber_hip_pt_history_download(None, p) == -1
    assert lib.amber_hip_pt_device_history(pt._h, None, None) == -1 and lib.amber_hip_pt_device_history(None, None, None) == -1
    with pytest.raises(amber.AmberError):
        pt.temporal(8, levels=9)
    with pytest.raises(amber.AmberError):
        pt.temporal(8, format=5)
    _, state, _ = T.temporal(state, fb, aov, 8, lens, sens, levels=0)
    assert np.array_equal(bits(pt.temporal(8, levels=0, format=amber.RESOLVE_MEAN_F32)), bits(state["hist"][..., :3])) and (pt.history_download()[..., 3] == 2).all()
    pt.close()


# ---- 5: the product library --------------------------------------------------------------------------------------------------------------------
PRODUCT_CHILD = r"""
import os, sys, json
sys.path.insert(0, {root!r})
import numpy as np
import amber_amd as A
assert A.library_path().name == "libamber_hip.so" and not A.is_lab()
pt = A.PathTracer(A.HostScene.cornell_box(), A.Sensor.default(64, 48), seed=5)
for frame in range(2):
    pt.clear(); pt.aov_clear(); pt.render_pass(frame * 16, 16); pt.aov_pass(frame * 16, 16)
    mean = pt.temporal(16, levels=2, k_color=0.0, format=A.RESOLVE_MEAN_F32)
np.save(os.path.join({tmp!r}, "mean.npy"), mean); np.save(os.path.join({tmp!r}, "history.npy"), pt.history_download())
pt.close()
print("RESULT " + json.dumps(dict(math=A.math_mode())))
"""


def test_product_library(amber, tmp_path):
    import os
    assert amber.is_lab()
    p = subprocess.run([sys.executable, "-c", PRODUCT_CHILD.format(root=str(ROOT), tmp=str(tmp_path))], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, AMBER_AMD_LIB="libamber_hip.so"))
    assert p.returncode == 0, p.stderr[-3000:]
    pt = amber.PathTracer(amber.HostScene.cornell_box(), amber.Sensor.default(64, 48), seed=5)
    for frame in range(2):
        pt.clear(); pt.aov_clear(); pt.render_pass(frame * 16, 16); pt.aov_pass(frame * 16, 16)
        mean = pt.temporal(16, levels=2, k_color=0.0, format=amber.RESOLVE_MEAN_F32)
    hist = pt.history_download()
    assert np.array_equal(bits(np.load(tmp_path / "mean.npy")), bits(mean)) and np.array_equal(bits(np.load(tmp_path / "history.npy")), bits(hist))
    assert mean.any() and hist[..., 3].max() == 2
    pt.close()

"""amber_hip_pt_denoise on the GPU (amber_amd/csrc/hip/denoise.inc): the edge-avoiding a-trous filter of the band's mean image, guided by the AOV buffer.

Every comparison of floats is exact equality of bits with tests/denoise_reference.py, the numpy restatement of the contract in include/amber_hip.h
(pinned on its own by tests/test_denoise_reference_cpu.py); the bytes are held to the host's amber.tonemap of those floats (skipped, as in
tests/test_resolve.py, in a portable-math measurement build, whose powf is not glibc's).
Shapes of the synthetic test, width x height: 1 x 1 (every tap but the centre outside), 1 x 40 (a column: every wave one lane), 37 x 23 (narrower than a
wave's row segment, and smaller than the level-4 reach of 32 pixels), 67 x 35 (a row of two segments, the second of three pixels; nine tile rows, the
last of three rows), 130 x 9 (three segments, a band lower than the level-2 reach).  levels 1, 2, 3, 5, 8: both parities of the ping-pong, and steps
(64, 128) beyond every one of these shapes."""
import ctypes
import functools
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import denoise_reference as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
N = 4
SPP = 64                                                                           # rendered frames: enough samples for the Cornell box's small light to be found
PARAMS = {"all zero": (0.0, 0.0, 0.0, 0.0), "defaults": (4.0, 100.0, 10.0, 0.25), "colour stop only": (0.0, 0.0, 0.0, 0.25)}
LEVELS = (1, 2, 3, 5, 8)
BPP = {0: 12, 1: 3, 2: 4}


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _hip():
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return hip


@functools.lru_cache(maxsize=None)
def synthetic(w, h):
    """(framebuffer sums, AOV sums) of N samples: a noisy two-colour image; coverage 0 .. 4 per pixel (a fifth of the pixels are misses), albedo
    constant over blocks of 7 x 5 pixels with neighbours 0.05 or 0.5 apart, a normal edge at the middle column, a depth step of a quarter at the
    middle row under a ripple of 2 %, and one pixel that was hit at depth 0"""
    rng = np.random.default_rng(100 * w + h)
    y, x = np.mgrid[0:h, 0:w]
    clean = np.where((x < w / 2)[..., None], F32([0.8, 0.2, 0.1]), F32([0.1, 0.3, 0.9]))
    fb = ((clean + rng.normal(0.0, 0.3, (h, w, 3))) * N).astype(F32)
    cov = rng.integers(0, 5, (h, w)).astype(F32)
    cov[0, min(w - 1, 3)] = 2
    albedo = np.array([0.7, 0.75, 0.2], F32)[(x // 7 + y // 5) % 3]
    normal = np.where((x < w / 2)[..., None], F32([0, 0, 1]), F32([0.6, 0, 0.8]))
    depth = (np.where(y < h / 2, 2.0, 2.5) * (1 + 0.02 * rng.random((h, w)))).astype(F32)
    depth[0, min(w - 1, 3)] = 0
    aov = np.zeros((h, w, 8), F32)
    aov[..., 0:3] = (albedo * cov)[..., None]
    aov[..., 3] = depth * cov
    aov[..., 4:7] = normal * cov[..., None]
    aov[..., 7] = cov
    return fb, aov


@functools.lru_cache(maxsize=None)
def reference(w, h, levels, k):
    fb, aov = synthetic(w, h)
    return R.denoise(fb, aov, N, levels, *k)


def upload(pt, fb, aov):
    """fb and aov into the handle's framebuffer and AOV buffer (device_aov allocates and zeroes it on the stream: waited for before the copy)"""
    fptr, n_floats = pt.device_framebuffer()
    aptr, n_pixels = pt.device_aov()
    pt.sync()
    assert n_floats == fb.size and n_pixels * 8 == aov.size
    hip = _hip()
    assert hip.hipMemcpy(fptr, fb.ctypes.data, fb.nbytes, 1) == 0 and hip.hipMemcpy(aptr, aov.ctypes.data, aov.nbytes, 1) == 0      # hipMemcpyHostToDevice
    assert np.array_equal(bits(pt.download()[0]), bits(fb)) and np.array_equal(bits(pt.aov_download()), bits(aov))


def kw(levels, k):
    return dict(levels=levels, k_normal=k[0], k_albedo=k[1], k_depth=k[2], k_color=k[3])


def cornell(amber, w=64, h=48, **kwargs):
    return amber.PathTracer(amber.HostScene.cornell_box(), amber.Sensor.default(w, h), **kwargs)


# ---- 1: synthetic inputs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (1, 40), (37, 23), (67, 35), (130, 9)])
def test_synthetic_inputs(amber, w, h):
    fb, aov = synthetic(w, h)
    assert (aov[..., 7] == 0).any() or w * h == 1
    pt = cornell(amber, w, h)
    upload(pt, fb, aov)
    glibc = amber.math_mode() == amber.MATH_GLIBC
    for what, k in PARAMS.items():
        for levels in LEVELS:
            want = reference(w, h, levels, k)
            assert np.isfinite(want).all()
            got = pt.denoise(N, format=amber.RESOLVE_MEAN_F32, **kw(levels, k))
            assert got.dtype == F32 and got.shape == (h, w, 3)
            wrong = int((bits(got) != bits(want)).any(axis=-1).sum())
            assert wrong == 0, (what, levels, f"{wrong} of {w * h} pixels differ")
            if levels not in (2, 5):
                continue
            assert np.array_equal(bits(pt.denoise(N, format=amber.RESOLVE_MEAN_F32, mirror=True, **kw(levels, k))), bits(want[:, ::-1])), (what, levels, "mirrored mean")
            if not glibc:
                continue
            ldr = amber.tonemap(want)
            for mirror in (False, True):
                flip = (lambda a: a[:, ::-1]) if mirror else (lambda a: a)
                rgb = pt.denoise(N, format=amber.RESOLVE_RGB8, mirror=mirror, **kw(levels, k))
                assert rgb.dtype == np.uint8 and np.array_equal(rgb, flip(ldr)), (what, levels, mirror, "rgb8")
                rgba = pt.denoise(N, format=amber.RESOLVE_RGBA8, mirror=mirror, **kw(levels, k))
                assert rgba.shape == (h, w, 4) and np.array_equal(rgba[..., :3], flip(ldr)) and (rgba[..., 3] == 255).all(), (what, levels, mirror, "rgba8")
    if w * h > 1:
        filtered = reference(w, h, 5, PARAMS["defaults"])
        assert not np.array_equal(filtered, fb / F32(N)) and not np.array_equal(filtered, reference(w, h, 5, PARAMS["all zero"]))    # the stops act
    pt.close()


def test_a_nan_pixel(amber):
    """0 * NaN is NaN: a NaN colour reaches every pixel that has it for a tap, whatever the tap's weight; positions equal, every other bit equal"""
    w, h = 67, 35
    fb, aov = synthetic(w, h)
    fb = fb.copy()
    fb[17, 30, 1] = np.nan
    pt = cornell(amber, w, h)
    upload(pt, fb, aov)
    for levels in (1, 2):
        want = R.denoise(fb, aov, N, levels, *PARAMS["defaults"])
        got = pt.denoise(N, format=amber.RESOLVE_MEAN_F32, **kw(levels, PARAMS["defaults"]))
        nan = np.isnan(want)
        assert nan[17, 30, 1] and 25 <= nan.sum() < want.size // 2
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan]), levels
    pt.close()


# ---- 2: a rendered frame, every engine ---------------------------------------------------------------------------------------------------------
def test_a_rendered_frame(amber):
    """4 samples: the frame the filter is meant for (in the Cornell box, whose light is small and found by chance, nearly all of it is still black);
    SPP samples: a frame with lit pixels on both sides of every edge"""
    for engine in (amber.ENGINE_AUTO, amber.ENGINE_BVH, amber.ENGINE_REFERENCE_BVH):
        for spp in (N, SPP):
            pt = cornell(amber, seed=5, engine=engine)
            pt.render_pass(0, spp)
            pt.aov_pass(0, spp)
            got = pt.denoise(spp, format=amber.RESOLVE_MEAN_F32)
            total, aov = pt.download()[0], pt.aov_download()
            want = R.denoise(total, aov, spp)
            assert (aov[..., 7] > 0).any() and (aov[..., 7] == 0).any()
            assert np.array_equal(bits(got), bits(want)), (engine, spp)
            # the Cornell box's light is found by chance: a low-sample frame is a few very bright pixels in black, which the colour stop
            # (rightly) keeps apart, so the guides alone (k_color = 0) are checked too -- there the bright pixels must spread
            guided = pt.denoise(spp, k_color=0.0, format=amber.RESOLVE_MEAN_F32)
            assert np.array_equal(bits(guided), bits(R.denoise(total, aov, spp, k_color=0.0))), (engine, spp, "k_color = 0")
            if spp == SPP:
                assert np.count_nonzero(total) > 0 and not np.array_equal(bits(guided), bits(total / F32(spp)))
            if amber.math_mode() == amber.MATH_GLIBC:
                assert np.array_equal(pt.denoise(spp), amber.tonemap(want)), (engine, spp)    # the default format is RGB8
            pt.close()


# ---- 3: bands --------------------------------------------------------------------------------------------------------------------------------
def test_bands(amber):
    lib = amber.load_library()
    pt = cornell(amber, seed=5, rows=(5, 29))
    pt.render_pass(0, SPP)
    pt.aov_pass(0, SPP)
    total, aov = pt.download()[0], pt.aov_download()
    assert total.shape == (24, 64, 3)
    assert np.array_equal(bits(pt.denoise(SPP, format=amber.RESOLVE_MEAN_F32)), bits(R.denoise(total, aov, SPP)))      # a band filters within itself
    pt.close()
    striped = cornell(amber, seed=5, rows=(2, 24), stripe=(2, 6))
    striped.render_pass(0, SPP)
    buf = np.full(8 * 64 * 3, 0xAB, np.uint8)
    params = amber.DenoiseParams(levels=5, k_normal=4.0, k_albedo=100.0, k_depth=10.0, k_color=0.25)
    assert len(striped.row_index) == 8
    assert lib.amber_hip_pt_denoise(striped._h, SPP, ctypes.byref(params), amber.RESOLVE_RGB8, buf.ctypes.data, buf.nbytes, amber.RESOLVE_HOST) == -1      # AMBER_EINVAL
    assert b"amber_hip_pt_denoise" in lib.amber_hip_last_error() and b"strip" in lib.amber_hip_last_error() and (buf == 0xAB).all()
    with pytest.raises(amber.AmberError):
        striped.denoise(SPP)
    assert striped.resolve(SPP).shape == (8, 64, 3)                                              # the handle works
    striped.close()
    empty = cornell(amber, seed=5, rows=(5, 5))
    for fmt in BPP:
        assert lib.amber_hip_pt_denoise(empty._h, SPP, ctypes.byref(params), fmt, None, 0, 0) == 0
        assert lib.amber_hip_pt_denoise(empty._h, SPP, ctypes.byref(params), fmt, None, 0, amber.RESOLVE_HOST | amber.RESOLVE_MIRROR_X) == 0
    assert empty.denoise(SPP).shape == (0, 64, 3)
    assert lib.amber_hip_pt_denoise(empty._h, SPP, ctypes.byref(params), amber.RESOLVE_RGB8, None, 3, 0) == -1     # the exact size holds for an empty band too
    empty.close()


# ---- 4: repeatability and what the call leaves alone ---------------------------------------------------------------------------------------------
def test_repeatable_and_buffers_are_reused(amber):
    """(k_color = 0: the guides alone, so that two and five levels differ on a frame of a few bright pixels)"""
    pt = cornell(amber, seed=2)
    pt.render_pass(0, SPP)
    pt.aov_pass(0, SPP)
    total, aov = pt.download()[0], pt.aov_download()
    five = pt.denoise(SPP, levels=5, k_color=0.0, format=amber.RESOLVE_MEAN_F32)
    assert np.array_equal(bits(five), bits(pt.denoise(SPP, levels=5, k_color=0.0, format=amber.RESOLVE_MEAN_F32)))
    two = pt.denoise(SPP, levels=2, k_color=0.0, format=amber.RESOLVE_MEAN_F32)
    assert np.array_equal(bits(two), bits(R.denoise(total, aov, SPP, levels=2, k_color=0.0))) and not np.array_equal(bits(two), bits(five))
    assert np.array_equal(bits(five), bits(pt.denoise(SPP, levels=5, k_color=0.0, format=amber.RESOLVE_MEAN_F32)))
    assert np.array_equal(bits(five), bits(R.denoise(total, aov, SPP, k_color=0.0)))
    pt.close()


def test_guides_never_filled_are_all_zero(amber):
    """no aov_* call before: the call allocates the buffer itself, and only the colour stop acts"""
    pt = cornell(amber, seed=2)
    pt.render_pass(0, SPP)
    got = pt.denoise(SPP, format=amber.RESOLVE_MEAN_F32)
    total = pt.download()[0]
    assert np.array_equal(bits(got), bits(R.denoise(total, np.zeros(total.shape[:2] + (8,), F32), SPP)))
    assert not pt.aov_download().any()
    pt.close()


def test_denoise_leaves_the_sums_the_aovs_the_ray_count_and_the_kernel_time_alone(amber):
    pt = cornell(amber, 40, 24, seed=2)
    pt.render_pass(0, SPP)
    pt.aov_pass(0, SPP)
    before, rays_before = pt.download()
    aov_before = pt.aov_download()
    time_before = pt.kernel_time()
    for fmt in BPP:
        for mirror in (False, True):
            pt.denoise(SPP, format=fmt, mirror=mirror)
    after, rays_after = pt.download()
    assert np.array_equal(bits(before), bits(after)) and rays_before == rays_after and rays_before > 0
    assert np.array_equal(bits(aov_before), bits(pt.aov_download())) and aov_before.any()
    assert pt.kernel_time() == time_before and time_before[0] >= 1
    pt.close()


# ---- 5: stream order -------------------------------------------------------------------------------------------------------------------------
TORCH_CHILD = r"""
import os, sys, json
sys.path.insert(0, {root!r})
import numpy as np
import torch
torch.cuda.init()
import amber_amd as A
dev = torch.device("cuda", 0)
W, H, SPP = 40, 24, 64
hs, sensor = A.HostScene.cornell_box(), A.Sensor.default(W, H)
ref = A.PathTracer(hs, sensor, seed=2)
ref.render_pass(0, SPP); ref.aov_pass(0, SPP); ref.sync()
want = ref.denoise(SPP, k_color=0.0, format=A.RESOLVE_RGBA8)
want_mean = ref.denoise(SPP, k_color=0.0, format=A.RESOLVE_MEAN_F32)
plain_resolve = ref.resolve(SPP, A.RESOLVE_RGBA8)
ref.clear(); ref.aov_clear(); ref.sync()
want_zero = ref.denoise(SPP, k_color=0.0, format=A.RESOLVE_RGBA8)
ref.close()
pt = A.PathTracer(hs, sensor, seed=2)
ext = torch.cuda.ExternalStream(pt.stream(), device=dev)
with torch.cuda.stream(ext):
    first = torch.full((H, W, 4), 7, dtype=torch.uint8, device=dev)
    second = torch.full((H, W, 4), 7, dtype=torch.uint8, device=dev)
    pt.render_pass(0, SPP)
    pt.aov_pass(0, SPP)
    returned = pt.denoise(SPP, k_color=0.0, format=A.RESOLVE_RGBA8, out=first)       # nothing waits between the passes, the filter and the clears
    pt.clear()
    pt.aov_clear()
    pt.denoise(SPP, k_color=0.0, format=A.RESOLVE_RGBA8, out=second)
    pt.sync()
out = dict(returned_out=returned is first, after_pass=bool(np.array_equal(first.cpu().numpy(), want)), picture=int(len(np.unique(want))),
           filtered=bool(not np.array_equal(want, plain_resolve)), after_clear=bool(np.array_equal(second.cpu().numpy(), want_zero)))
out["zero_rgb"] = sorted(set(want_zero[..., :3].reshape(-1).tolist())); out["zero_alpha"] = sorted(set(want_zero[..., 3].reshape(-1).tolist()))
# torch's current stream instead of the handle's: the binding orders the two itself
plain = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
pt.render_pass(0, SPP)
pt.aov_pass(0, SPP)
pt.denoise(SPP, k_color=0.0, format=A.RESOLVE_RGBA8, out=plain)
out["current_stream"] = bool(np.array_equal(plain.cpu().numpy(), want))
mean = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
pt.denoise(SPP, k_color=0.0, format=A.RESOLVE_MEAN_F32, mirror=True, out=mean)
out["mean_mirror"] = bool(np.array_equal(mean.cpu().numpy().view(np.uint32), want_mean[:, ::-1].view(np.uint32)))
refused = []
for bad in (torch.empty((H, W, 3), dtype=torch.uint8, device=dev), torch.empty((H, W, 4), dtype=torch.float32, device=dev), torch.empty((H, W, 8), dtype=torch.uint8, device=dev)[..., :4],
            torch.empty((H, W, 4), dtype=torch.uint8)):
    try:
        pt.denoise(SPP, k_color=0.0, format=A.RESOLVE_RGBA8, out=bad); refused.append(False)
    except A.AmberError:
        refused.append(True)
out["refused"] = refused
pt.close()
print("RESULT " + json.dumps(out))
"""


def _child(script, env=None, **fmt):
    p = subprocess.run([sys.executable, "-c", script.format(root=str(ROOT), **fmt)], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][7:])


def test_stream_order_into_a_torch_tensor(amber):
    """render_pass, aov_pass, denoise into a device tensor, both clears, denoise again, one sync at the end: the first tensor holds the filtered
    pass, the second the bytes of an all-zero image"""
    res = _child(TORCH_CHILD)
    assert res["returned_out"] and res["after_pass"] and res["picture"] >= 2 and res["filtered"], res
    assert res["after_clear"] and res["zero_rgb"] == [0] and res["zero_alpha"] == [255], res
    assert res["current_stream"] and res["mean_mirror"], res
    assert res["refused"] == [True, True, True, True], res


# ---- 6: errors ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_are_einval_and_leave_the_handle_working(amber):
    lib = amber.load_library()
    pt = cornell(amber, 20, 6, seed=1)
    pt.render_pass(0, 8)
    pt.aov_pass(0, 8)
    good = pt.denoise(8, format=amber.RESOLVE_RGBA8)
    HOST = amber.RESOLVE_HOST
    buf = np.full(20 * 6 * 12 + 64, 0xAB, np.uint8)
    p = buf.ctypes.data

    def P(**over):
        f = dict(levels=5, k_normal=4.0, k_albedo=100.0, k_depth=10.0, k_color=0.25)
        reserved = over.pop("reserved", (0, 0, 0))
        f.update(over)
        return ctypes.byref(amber.DenoiseParams(reserved=(ctypes.c_uint32 * 3)(*reserved), **f))
    cases = {"null handle": (None, 8, P(), 1, p, 360, HOST), "null params": (pt._h, 8, None, 1, p, 360, HOST), "n_samples == 0": (pt._h, 0, P(), 1, p, 360, HOST),
             "levels 0": (pt._h, 8, P(levels=0), 1, p, 360, HOST), "levels 9": (pt._h, 8, P(levels=9), 1, p, 360, HOST),
             "unknown format": (pt._h, 8, P(), 3, p, 360, HOST), "unknown flag bits": (pt._h, 8, P(), 1, p, 360, HOST | 4),
             "null out": (pt._h, 8, P(), 1, None, 360, HOST), "null out, device": (pt._h, 8, P(), 1, None, 360, 0),
             "one byte short": (pt._h, 8, P(), 1, p, 359, HOST), "one byte long": (pt._h, 8, P(), 1, p, 361, HOST), "RGBA8 size for RGB8": (pt._h, 8, P(), 1, p, 480, HOST),
             "RGB8 size for RGBA8": (pt._h, 8, P(), 2, p, 360, HOST), "RGB8 size for the mean": (pt._h, 8, P(), 0, p, 360, HOST), "zero bytes": (pt._h, 8, P(), 1, p, 0, HOST)}
    for i in range(3):
        cases[f"reserved[{i}]"] = (pt._h, 8, P(reserved=[int(j == i) for j in range(3)]), 1, p, 360, HOST)
    for field in ("k_normal", "k_albedo", "k_depth", "k_color"):
        for bad in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
            cases[f"{field} = {bad}"] = (pt._h, 8, P(**{field: bad}), 1, p, 360, HOST)
    for what, args in cases.items():
        assert lib.amber_hip_pt_denoise(*args) == -1, what                                # AMBER_EINVAL
        assert b"amber_hip_pt_denoise" in lib.amber_hip_last_error(), what
        assert (buf == 0xAB).all(), what                                                   # no effect
    with pytest.raises(amber.AmberError):
        pt.denoise(8, format=5)
    with pytest.raises(amber.AmberError):
        pt.denoise(8, levels=0)
    assert np.array_equal(pt.denoise(8, format=amber.RESOLVE_RGBA8), good)
    pt.render_pass(8, 120)                                                                   # and the handle renders afterwards
    pt.aov_pass(8, 120)
    assert np.array_equal(bits(pt.denoise(128, format=amber.RESOLVE_MEAN_F32)), bits(R.denoise(pt.download()[0], pt.aov_download(), 128)))
    pt.close()


# ---- 7: the product library --------------------------------------------------------------------------------------------------------------------
PRODUCT_CHILD = r"""
import os, sys, json
sys.path.insert(0, {root!r})
import numpy as np
import amber_amd as A
assert A.library_path().name == "libamber_hip.so" and not A.is_lab()
pt = A.PathTracer(A.HostScene.cornell_box(), A.Sensor.default(64, 48), seed=5)
pt.render_pass(0, 64); pt.aov_pass(0, 64)
np.save(os.path.join({tmp!r}, "mean.npy"), pt.denoise(64, format=A.RESOLVE_MEAN_F32)); np.save(os.path.join({tmp!r}, "rgb8.npy"), pt.denoise(64))
pt.close()
print("RESULT " + json.dumps(dict(math=A.math_mode())))
"""


def test_product_library(amber, tmp_path):
    assert amber.is_lab()
    res = _child(PRODUCT_CHILD, env=dict(os.environ, AMBER_AMD_LIB="libamber_hip.so"), tmp=str(tmp_path))
    assert res["math"] == amber.MATH_GLIBC
    pt = cornell(amber, seed=5)
    pt.render_pass(0, SPP)
    pt.aov_pass(0, SPP)
    mean = pt.denoise(SPP, format=amber.RESOLVE_MEAN_F32)
    assert np.array_equal(bits(np.load(tmp_path / "mean.npy")), bits(mean)) and np.array_equal(bits(mean), bits(R.denoise(pt.download()[0], pt.aov_download(), SPP))) and mean.any()
    if amber.math_mode() == amber.MATH_GLIBC:
        assert np.array_equal(np.load(tmp_path / "rgb8.npy"), pt.denoise(64))
    pt.close()

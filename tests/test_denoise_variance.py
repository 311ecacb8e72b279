"""amber_hip_pt_denoise_variance on the GPU (amber_amd/csrc/hip/denoise_variance.inc): the a-trous filter whose luminance stop is scaled by the variance
of the mean, which comes from the batch moments and is filtered along with the colour.

Every comparison of floats is exact equality of bits with tests/denoise_variance_reference.py, the numpy restatement of the contract in
include/amber_hip.h (pinned on its own by tests/test_denoise_variance_reference_cpu.py); where the restatement has a NaN the device must have one and
every other value equal bits.  The bytes are held to the host's amber.tonemap of those floats (skipped, as in tests/test_denoise.py, in a portable-math
measurement build).  The shapes of the synthetic test are tests/test_denoise.py's, for the reasons that file gives: 1 x 1, 1 x 40, 37 x 23, 67 x 35,
130 x 9.  levels 1, 2, 5, 8: both parities of the ping-pong, the last level's 12-byte output after an even and an odd number of record levels, and steps
(64, 128) beyond every shape.  var_radius 0, 1, 3: no pool, the smallest, the largest.  The mirrored mean and the RGB8 / RGBA8 bytes are checked
at levels 2 and 5 with var_radius 3 only: the output stage is resolve's kernel on the last colour buffer whatever the radius, and the means that feed it
are compared for every radius."""
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
import denoise_variance_reference as V
from test_moments import light_room

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
N = 4
PARAMS = {"all zero": (0.0, 0.0, 0.0, 0.0), "defaults": (4.0, 100.0, 10.0, 16.0), "k_lum only": (0.0, 0.0, 0.0, 16.0)}
LEVELS = (1, 2, 5, 8)
RADII = (0, 1, 3)
SHAPES = [(1, 1), (1, 40), (37, 23), (67, 35), (130, 9)]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same(got, want):
    """NaN where the restatement has NaN, the restatement's bits everywhere else"""
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def _hip():
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    return hip


@functools.lru_cache(maxsize=None)
def synthetic(w, h):
    """(framebuffer sums, AOV sums, moments) of N samples in up to N batches of one: tests/test_denoise.py's noisy two-colour image and guides (coverage
    0 .. 4, albedo blocks, a normal edge, a depth step, a pixel hit at depth 0); every pixel has 0 .. 4 batches (a fifth have none) whose luminances
    scatter around the clean image's; and, except in the band of one pixel, one pixel whose green sum is NaN"""
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
    batches = rng.integers(0, 5, (h, w))
    moments = np.zeros((h, w, 4), F32)
    for k in range(4):
        lum = np.abs(V.lum(clean) + rng.normal(0.0, 0.3, (h, w))).astype(F32)
        live = batches > k
        moments[..., 0] = np.where(live, moments[..., 0] + lum, moments[..., 0])
        moments[..., 1] = np.where(live, moments[..., 1] + lum * lum, moments[..., 1])
    moments[..., 2] = batches
    if w * h > 1:
        fb[h // 2, w // 2, 1] = np.nan
    return fb, aov, moments


@functools.lru_cache(maxsize=None)
def reference(w, h, levels, k, radius):
    fb, aov, moments = synthetic(w, h)
    return V.denoise_variance(fb, aov, moments, N, levels, *k, radius)


def upload(pt, fb, aov, moments):
    """the three inputs into the handle's buffers (device_aov / device_moments allocate and zero theirs on the stream: waited for before the copies)"""
    fptr, n_floats = pt.device_framebuffer()
    aptr, n_pixels = pt.device_aov()
    mptr, m_pixels = pt.device_moments()
    pt.sync()
    assert n_floats == fb.size and n_pixels * 8 == aov.size and m_pixels * 4 == moments.size
    hip = _hip()
    for ptr, a in ((fptr, fb), (aptr, aov), (mptr, moments)):
        assert hip.hipMemcpy(ptr, a.ctypes.data, a.nbytes, 1) == 0                  # hipMemcpyHostToDevice
    assert same(pt.download()[0], fb) and np.array_equal(bits(pt.aov_download()), bits(aov)) and np.array_equal(bits(pt.moments_download()), bits(moments))


def kw(levels, k, radius):
    return dict(levels=levels, k_normal=k[0], k_albedo=k[1], k_depth=k[2], k_lum=k[3], var_radius=radius)


def cornell(amber, w=64, h=48, **kwargs):
    return amber.PathTracer(amber.HostScene.cornell_box(), amber.Sensor.default(w, h), **kwargs)


# ---- 1: synthetic inputs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SHAPES)
def test_synthetic_inputs(amber, w, h):
    fb, aov, moments = synthetic(w, h)
    if w * h > 1:
        assert (aov[..., 7] == 0).any() and (moments[..., 2] == 0).any() and np.isnan(fb).sum() == 1
    pt = cornell(amber, w, h)
    upload(pt, fb, aov, moments)
    glibc = amber.math_mode() == amber.MATH_GLIBC
    for what, k in PARAMS.items():
        for levels in LEVELS:
            for radius in RADII:
                want = reference(w, h, levels, k, radius)
                got = pt.denoise_variance(N, format=amber.RESOLVE_MEAN_F32, **kw(levels, k, radius))       # (out=None: the AMBER_RESOLVE_HOST path)
                assert got.dtype == F32 and got.shape == (h, w, 3)
                assert same(got, want), (what, levels, radius, f"{int((bits(got) != bits(want)).any(axis=-1).sum())} of {w * h} pixels differ")
                if levels not in (2, 5) or radius != 3:
                    continue
                assert same(pt.denoise_variance(N, format=amber.RESOLVE_MEAN_F32, mirror=True, **kw(levels, k, radius)), want[:, ::-1]), (what, levels, "mirrored mean")
                if not glibc:
                    continue
                ldr = amber.tonemap(want)
                for mirror in (False, True):
                    flip = (lambda a: a[:, ::-1]) if mirror else (lambda a: a)
                    rgb = pt.denoise_variance(N, format=amber.RESOLVE_RGB8, mirror=mirror, **kw(levels, k, radius))
                    assert rgb.dtype == np.uint8 and np.array_equal(rgb, flip(ldr)), (what, levels, mirror, "rgb8")
                    rgba = pt.denoise_variance(N, format=amber.RESOLVE_RGBA8, mirror=mirror, **kw(levels, k, radius))
                    assert rgba.shape == (h, w, 4) and np.array_equal(rgba[..., :3], flip(ldr)) and (rgba[..., 3] == 255).all(), (what, levels, mirror, "rgba8")
    if w * h > 1:
        d = [reference(w, h, 5, PARAMS["defaults"], r) for r in RADII]
        mean = fb / F32(N)
        assert not same(d[2], mean) and not same(d[0], d[2]) and not same(d[1], d[2])                        # the filter acts, and the pool matters
        assert not same(d[2], reference(w, h, 5, PARAMS["k_lum only"], 3))                                   # ... and so do the guide stops
        if w * h > 40:                                                                                       # the NaN stays local (1 x 40: every pixel is within five levels' reach)
            assert 25 <= np.isnan(reference(w, h, 2, PARAMS["defaults"], 3)).any(axis=-1).sum() <= 13 * 13
    pt.close()


def test_a_device_pointer(amber):
    """without AMBER_RESOLVE_HOST out is device memory and the call is stream-ordered: read after sync()"""
    w, h = 67, 35
    fb, aov, moments = synthetic(w, h)
    pt = cornell(amber, w, h)
    upload(pt, fb, aov, moments)
    lib, hip = amber.load_library(), _hip()
    params = amber.DenoiseVarianceParams(**kw(5, PARAMS["defaults"], 3))
    dev = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(dev), w * h * 12) == 0
    try:
        for mirror in (0, amber.RESOLVE_MIRROR_X):
            assert lib.amber_hip_pt_denoise_variance(pt._h, N, ctypes.byref(params), amber.RESOLVE_MEAN_F32, dev, w * h * 12, mirror) == 0
            pt.sync()
            got = np.empty((h, w, 3), F32)
            assert hip.hipMemcpy(got.ctypes.data, dev, got.nbytes, 2) == 0           # hipMemcpyDeviceToHost
            want = reference(w, h, 5, PARAMS["defaults"], 3)
            assert same(got, want[:, ::-1] if mirror else want), mirror
    finally:
        hip.hipFree(dev)
    pt.close()


# ---- 2: a rendered frame -----------------------------------------------------------------------------------------------------------------------
def rendered(amber, pt):
    """four batches of one sample, the guides of the same samples, the filter; the restatement fed with the three downloads"""
    for s in range(N):
        pt.render_batch(s, 1)
    pt.aov_pass(0, N)
    got = pt.denoise_variance(N, format=amber.RESOLVE_MEAN_F32)
    total, aov, moments = pt.download()[0], pt.aov_download(), pt.moments_download()
    assert (moments[..., 2] == N).all()
    return got, V.denoise_variance(total, aov, moments, N), total, aov, moments


def test_a_rendered_frame(amber):
    room = amber.HostScene.create_arrays(**light_room())
    for engine in (amber.ENGINE_AUTO, amber.ENGINE_BVH):
        pt = cornell(amber, seed=5, engine=engine)                                  # the frame the filter is meant for: a few bright pixels in black
        got, want, total, aov, moments = rendered(amber, pt)
        assert np.array_equal(bits(got), bits(want)), engine
        assert (aov[..., 7] > 0).any() and (aov[..., 7] == 0).any()
        if amber.math_mode() == amber.MATH_GLIBC:
            assert np.array_equal(pt.denoise_variance(N), amber.tonemap(want)), engine                      # the default format is RGB8
        pt.close()
        pt = amber.PathTracer(room, amber.Sensor.default(64, 48), seed=5, engine=engine)                    # a frame with light, and so moments, in most pixels
        got, want, total, aov, moments = rendered(amber, pt)
        assert np.array_equal(bits(got), bits(want)) and np.isfinite(want).all(), engine
        assert (moments[..., 1] > 0).mean() >= 0.5 and not np.array_equal(bits(want), bits(total / F32(N)))
        assert not np.array_equal(bits(want), bits(R.denoise(total, aov, N)))
        pt.close()


PRODUCT_CHILD = r"""
import os, sys, json
sys.path.insert(0, {root!r})
sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import amber_amd as A
from test_moments import light_room
assert A.library_path().name == "libamber_hip.so" and not A.is_lab()
for name, hs in (("cornell", A.HostScene.cornell_box()), ("room", A.HostScene.create_arrays(**light_room()))):
    for engine in (A.ENGINE_AUTO, A.ENGINE_BVH):
        pt = A.PathTracer(hs, A.Sensor.default(64, 48), seed=5, engine=engine)
        for s in range(4):
            pt.render_batch(s, 1)
        pt.aov_pass(0, 4)
        np.save(os.path.join({tmp!r}, "%s_%d_mean.npy" % (name, engine)), pt.denoise_variance(4, format=A.RESOLVE_MEAN_F32))
        np.save(os.path.join({tmp!r}, "%s_%d_moments.npy" % (name, engine)), pt.moments_download())
        pt.close()
print("RESULT " + json.dumps(dict(math=A.math_mode())))
"""


def test_product_library(amber, tmp_path):
    assert amber.is_lab()
    p = subprocess.run([sys.executable, "-c", PRODUCT_CHILD.format(root=str(ROOT), tmp=str(tmp_path))], capture_output=True, text=True,
                       env=dict(os.environ, AMBER_AMD_LIB="libamber_hip.so"), timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    assert res["math"] == amber.MATH_GLIBC
    for name, hs in (("cornell", amber.HostScene.cornell_box()), ("room", amber.HostScene.create_arrays(**light_room()))):
        for engine in (amber.ENGINE_AUTO, amber.ENGINE_BVH):
            pt = amber.PathTracer(hs, amber.Sensor.default(64, 48), seed=5, engine=engine)
            got, want, _, _, moments = rendered(amber, pt)
            assert np.array_equal(bits(np.load(tmp_path / f"{name}_{engine}_moments.npy")), bits(moments)), (name, engine)
            assert np.array_equal(bits(np.load(tmp_path / f"{name}_{engine}_mean.npy")), bits(want)) and np.array_equal(bits(got), bits(want)), (name, engine)
            pt.close()


# ---- 3: repeatability and what the call leaves alone -------------------------------------------------------------------------------------------
def test_repeatable_and_leaves_everything_else_alone(amber):
    pt = amber.PathTracer(amber.HostScene.create_arrays(**light_room()), amber.Sensor.default(40, 24), seed=2)
    for s in range(N):
        pt.render_batch(s, 1)
    pt.aov_pass(0, N)
    plain_before = {fmt: pt.denoise(N, format=fmt) for fmt in (amber.RESOLVE_MEAN_F32, amber.RESOLVE_RGB8, amber.RESOLVE_RGBA8)}
    before, rays_before = pt.download()
    aov_before, moments_before, time_before = pt.aov_download(), pt.moments_download(), pt.kernel_time()
    five = pt.denoise_variance(N, format=amber.RESOLVE_MEAN_F32)
    assert np.array_equal(bits(five), bits(pt.denoise_variance(N, format=amber.RESOLVE_MEAN_F32)))
    two = pt.denoise_variance(N, levels=2, var_radius=1, format=amber.RESOLVE_MEAN_F32)
    assert np.array_equal(bits(two), bits(V.denoise_variance(before, aov_before, moments_before, N, levels=2, var_radius=1))) and not np.array_equal(bits(two), bits(five))
    for fmt in (amber.RESOLVE_MEAN_F32, amber.RESOLVE_RGB8, amber.RESOLVE_RGBA8):
        for mirror in (False, True):
            pt.denoise_variance(N, format=fmt, mirror=mirror)
    assert np.array_equal(bits(five), bits(pt.denoise_variance(N, format=amber.RESOLVE_MEAN_F32)))
    assert np.array_equal(bits(five), bits(V.denoise_variance(before, aov_before, moments_before, N)))
    after, rays_after = pt.download()
    assert np.array_equal(bits(before), bits(after)) and rays_before == rays_after and rays_before > 0
    assert np.array_equal(bits(aov_before), bits(pt.aov_download())) and aov_before.any()
    assert np.array_equal(bits(moments_before), bits(pt.moments_download())) and moments_before.any()
    assert pt.kernel_time() == time_before and time_before[0] >= N
    for fmt, want in plain_before.items():                                            # the two filters share a colour buffer and the guide buffer
        assert np.array_equal(pt.denoise(N, format=fmt).view(np.uint8), want.view(np.uint8)), fmt
    pt.close()


def test_moments_never_filled_are_all_zero(amber):
    """no render_batch, no moments_* call before: the call allocates the buffer itself; without batches every var is 0, r = 1e10, and only taps of
    equal luminance pass"""
    pt = cornell(amber, seed=2)
    pt.render_pass(0, 64)
    pt.aov_pass(0, 64)
    got = pt.denoise_variance(64, format=amber.RESOLVE_MEAN_F32)
    total, aov = pt.download()[0], pt.aov_download()
    assert np.array_equal(bits(got), bits(V.denoise_variance(total, aov, np.zeros(total.shape[:2] + (4,), F32), 64))) and total.any()
    assert not pt.moments_download().any()
    pt.close()

"""amber_hip_pt_resolve on the GPU (amber_amd/csrc/hip/resolve.inc): the framebuffer's sums as the mean, or through Filmic + Gamma 2.2 as 8-bit RGB /
RGBA, in device memory.

Every comparison is exact equality.  The bytes are held to oracle_tonemap (the checker the host's output stage is held to, tests/test_output_stage.py)
and to the host's own amber.tonemap; the floats to numpy's binary32 division, as uint32 views.  Byte comparisons are skipped in a portable-math
measurement build (its powf is not glibc's); the mean is compared in every build.
Shapes of the chosen-image test, width x height: 1 x 1 (a tail only), 3 x 5 (15 pixels: three whole groups and a tail; width < 4, so every mirrored
group crosses a row end), 53 x 37 (odd width: mirrored loads at every dword phase, groups across row ends, a one-pixel tail; 491 groups in two
workgroups), 64 x 4 (width % 4 == 0: exactly one wave of groups, no tail, the aligned mirror), 257 x 3 (width % 4 == 1, a three-pixel tail).
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
from amber_amd import scenes

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
BPP = {0: 12, 1: 3, 2: 4}


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def mean_of(img, n):
    with np.errstate(all="ignore"):
        return (np.ascontiguousarray(img, F32) / F32(n)).astype(F32)


def need_glibc(amber):
    if amber.math_mode() != amber.MATH_GLIBC:
        pytest.skip("byte equality is the contract of the product's arithmetic (AMBER_MATH_GLIBC)")


def check_all_formats(amber, pt, img, n, what):
    """all three formats, mirrored and not, of a handle whose framebuffer holds img, against the oracle and numpy"""
    mean = mean_of(img, n)
    want = O.tonemap(mean) if amber.math_mode() == amber.MATH_GLIBC else None
    for mirror in (False, True):
        flip = (lambda a: a[:, ::-1]) if mirror else (lambda a: a)
        got = pt.resolve(n, amber.RESOLVE_MEAN_F32, mirror=mirror)
        assert got.dtype == F32 and got.shape == mean.shape
        assert np.array_equal(bits(got), bits(flip(mean))), (what, n, mirror, "mean")
        if want is None:
            continue
        rgb = pt.resolve(n, amber.RESOLVE_RGB8, mirror=mirror)
        assert rgb.dtype == np.uint8 and rgb.shape == want.shape
        assert np.array_equal(rgb, flip(want)), (what, n, mirror, "rgb8", int((rgb != flip(want)).sum()))
        rgba = pt.resolve(n, amber.RESOLVE_RGBA8, mirror=mirror)
        assert rgba.dtype == np.uint8 and rgba.shape == want.shape[:2] + (4,)
        assert np.array_equal(rgba[..., :3], flip(want)) and (rgba[..., 3] == 255).all(), (what, n, mirror, "rgba8")


# ---- 1: a rendered frame ---------------------------------------------------------------------------------------------------------------------
def test_a_rendered_frame(amber):
    need_glibc(amber)
    pt = amber.PathTracer(amber.HostScene.cornell_box(), amber.Sensor.default(72, 48), seed=5)
    pt.render_pass(0, 16)
    total, _ = pt.download()
    mean = total / F32(16)
    rgb = pt.resolve(16, amber.RESOLVE_RGB8)
    assert np.array_equal(rgb, O.tonemap(mean))
    assert np.array_equal(rgb, amber.tonemap(mean))
    assert rgb.max() > 0 and 0 < np.count_nonzero(rgb) < rgb.size                        # lit and unlit pixels, not a constant
    assert np.array_equal(bits(pt.resolve(16, amber.RESOLVE_MEAN_F32)), bits(mean))
    rgba = pt.resolve(16, amber.RESOLVE_RGBA8)
    assert np.array_equal(rgba[..., :3], rgb) and (rgba[..., 3] == 255).all()
    for fmt in (amber.RESOLVE_MEAN_F32, amber.RESOLVE_RGB8, amber.RESOLVE_RGBA8):
        assert np.array_equal(pt.resolve(16, fmt, mirror=True), pt.resolve(16, fmt)[:, ::-1]), fmt
    assert np.array_equal(pt.resolve(16), rgb)                                             # the default format is RGB8
    pt.close()


# ---- 2: the whole curve and the special values, at shapes where the grouping breaks -------------------------------------------------------------
SPECIALS = np.array([[0, 0, 0], [1e11, 1e11, 1e11], [1e-9, 0.0437, 0.7 / 16], [np.nan, -1.0, np.inf], [-0.0, 1e-30, 3e38],
                     [1e-40, -1e-30, 1.4e-45]], F32)      # tests/test_output_stage.py:58-59, then two subnormals and -1e-30


def _hip():
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return hip


def chosen_image(w, h):
    rng = np.random.default_rng(1000 * w + h)
    img = (1e-9 + (10.0 - 1e-9) * rng.random((h, w, 3)) ** 6).astype(F32)                # the whole curve: 1e-9 .. 10
    k = min(len(SPECIALS), w * h)
    img.reshape(-1, 3)[:k] = SPECIALS[:k]
    return img


@pytest.mark.parametrize("w,h", [(1, 1), (3, 5), (53, 37), (64, 4), (257, 3)])
def test_chosen_images_and_special_values(amber, w, h):
    pt = amber.PathTracer(amber.HostScene.cornell_box(), amber.Sensor.default(w, h))
    pt.sync()
    ptr, n_floats = pt.device_framebuffer()
    img = chosen_image(w, h)
    assert n_floats == img.size
    assert _hip().hipMemcpy(ptr, img.ctypes.data, img.nbytes, 1) == 0                     # hipMemcpyHostToDevice
    back, _ = pt.download()
    assert np.array_equal(bits(back), bits(img))
    if w * h >= len(SPECIALS) and amber.math_mode() == amber.MATH_GLIBC:                  # the rule the header states: negative, NaN, infinite -> 255
        assert pt.resolve(1).reshape(-1, 3)[3].tolist() == [255, 255, 255] and pt.resolve(1).reshape(-1, 3)[0].tolist() == [0, 0, 0]
    for n in (1, 7):
        check_all_formats(amber, pt, img, n, (w, h))
    pt.close()


# ---- 3: bands ------------------------------------------------------------------------------------------------------------------------------
def test_bands_and_stripes(amber):
    need_glibc(amber)
    hs, sensor = amber.HostScene.cornell_box(), amber.Sensor.default(40, 24)
    full = amber.PathTracer(hs, sensor, seed=9)
    full.render_pass(0, 8)
    want = full.resolve(8)
    assert np.array_equal(want, O.tonemap(full.download()[0] / F32(8)))
    full.close()
    for kw in (dict(rows=(8, 20)), dict(rows=(2, 24), stripe=(2, 6))):
        pt = amber.PathTracer(hs, sensor, seed=9, **kw)
        pt.render_pass(0, 8)
        got = pt.resolve(8)
        assert got.shape == (len(pt.row_index), 40, 3) and len(pt.row_index) in (12, 8)
        assert np.array_equal(got, want[pt.row_index]), kw
        assert np.array_equal(pt.resolve(8, mirror=True), want[pt.row_index][:, ::-1]), kw
        pt.close()
    empty = amber.PathTracer(hs, sensor, seed=9, rows=(5, 5))
    lib = amber.load_library()
    for fmt in BPP:
        assert lib.amber_hip_pt_resolve(empty._h, 8, fmt, None, 0, 0) == 0
        assert lib.amber_hip_pt_resolve(empty._h, 8, fmt, None, 0, amber.RESOLVE_HOST | amber.RESOLVE_MIRROR_X) == 0
    assert empty.resolve(8).shape == (0, 40, 3)
    assert lib.amber_hip_pt_resolve(empty._h, 8, amber.RESOLVE_RGB8, None, 3, 0) == -1     # the exact size holds for an empty band too
    empty.close()


# ---- 4: order and side effects ---------------------------------------------------------------------------------------------------------------
def test_resolve_leaves_the_sums_the_ray_count_and_the_kernel_time_alone(amber):
    pt = amber.PathTracer(amber.HostScene.cornell_box(), amber.Sensor.default(40, 24), seed=2)
    pt.render_pass(0, 16)
    before, rays_before = pt.download()
    time_before = pt.kernel_time()
    for fmt in BPP:
        for mirror in (False, True):
            pt.resolve(16, fmt, mirror=mirror)
    after, rays_after = pt.download()
    assert np.array_equal(bits(before), bits(after)) and rays_before == rays_after and rays_before > 0
    assert pt.kernel_time() == time_before and time_before[0] >= 1
    pt.close()


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
ref = A.PathTracer(hs, sensor, seed=2)
ref.render_pass(0, SPP); ref.sync()
want = ref.resolve(SPP, A.RESOLVE_RGBA8)
ref.clear(); ref.sync()
want_zero = ref.resolve(SPP, A.RESOLVE_RGBA8)
ref.close()
pt = A.PathTracer(hs, sensor, seed=2)
ext = torch.cuda.ExternalStream(pt.stream(), device=dev)
with torch.cuda.stream(ext):
    first = torch.full((H, W, 4), 7, dtype=torch.uint8, device=dev)
    second = torch.full((H, W, 4), 7, dtype=torch.uint8, device=dev)
    pt.render_pass(0, SPP)
    returned = pt.resolve(SPP, A.RESOLVE_RGBA8, out=first)       # nothing waits between the pass, the resolve and the clear
    pt.clear()
    pt.resolve(SPP, A.RESOLVE_RGBA8, out=second)
    pt.sync()
out = dict(returned_out=returned is first, after_pass=bool(np.array_equal(first.cpu().numpy(), want)), picture=int(len(np.unique(want))),
           after_clear=bool(np.array_equal(second.cpu().numpy(), want_zero)))
out["zero_rgb"] = sorted(set(want_zero[..., :3].reshape(-1).tolist())); out["zero_alpha"] = sorted(set(want_zero[..., 3].reshape(-1).tolist()))
# torch's current stream instead of the handle's: the binding orders the two itself
plain = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
pt.render_pass(0, SPP)
pt.resolve(SPP, A.RESOLVE_RGBA8, out=plain)
out["current_stream"] = bool(np.array_equal(plain.cpu().numpy(), want))
mean = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
pt.resolve(SPP, A.RESOLVE_MEAN_F32, mirror=True, out=mean)
out["mean_mirror"] = bool(np.array_equal(mean.cpu().numpy().view(np.uint32), (pt.download()[0] / np.float32(SPP))[:, ::-1].view(np.uint32)))
refused = []
for bad in (torch.empty((H, W, 3), dtype=torch.uint8, device=dev), torch.empty((H, W, 4), dtype=torch.float32, device=dev), torch.empty((H, W, 8), dtype=torch.uint8, device=dev)[..., :4],
            torch.empty((H, W, 4), dtype=torch.uint8)):
    try:
        pt.resolve(SPP, A.RESOLVE_RGBA8, out=bad); refused.append(False)
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
    """render_pass, resolve into a device tensor, clear, resolve again, one sync at the end: the first tensor holds the pass, the second the
    bytes of an all-zero image"""
    res = _child(TORCH_CHILD)
    assert res["returned_out"] and res["after_pass"] and res["picture"] >= 2, res
    assert res["after_clear"] and res["zero_rgb"] == [0] and res["zero_alpha"] == [255], res
    assert res["current_stream"] and res["mean_mirror"], res
    assert res["refused"] == [True, True, True, True], res


# ---- 5: every engine ---------------------------------------------------------------------------------------------------------------------------
def test_every_engine(amber):
    need_glibc(amber)
    kw = scenes.random_spheres(100, 7)
    kw["material_index"][:10] = 0                     # ten emitters (2 % of a hundred spheres may be none): a picture, not a black frame
    spheres = amber.HostScene.create_arrays(**kw)
    for hs, engine in ((amber.HostScene.cornell_box(), amber.ENGINE_AUTO), (spheres, amber.ENGINE_BVH), (spheres, amber.ENGINE_REFERENCE_BVH)):
        pt = amber.PathTracer(hs, amber.Sensor.default(72, 48), seed=5, engine=engine)     # (test 1's frame: lit and unlit pixels)
        pt.render_pass(0, 16)
        total, _ = pt.download()
        print(f"engine {engine}: {np.count_nonzero(total)} of {total.size} sums are not zero")
        assert np.array_equal(pt.resolve(16), O.tonemap(total / F32(16))), engine
        assert np.array_equal(bits(pt.resolve(16, amber.RESOLVE_MEAN_F32)), bits(total / F32(16))), engine
        pt.close()


# ---- 6: errors ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_are_einval_and_leave_the_handle_working(amber):
    lib = amber.load_library()
    pt = amber.PathTracer(amber.HostScene.cornell_box(), amber.Sensor.default(20, 6), seed=1)
    pt.render_pass(0, 8)
    good = pt.resolve(8, amber.RESOLVE_RGBA8)
    HOST = amber.RESOLVE_HOST
    buf = np.full(20 * 6 * 12 + 64, 0xAB, np.uint8)
    p = buf.ctypes.data
    cases = {"null handle": (None, 8, 1, p, 360, HOST), "n_samples == 0": (pt._h, 0, 1, p, 360, HOST), "unknown format": (pt._h, 8, 3, p, 360, HOST),
             "unknown flag bits": (pt._h, 8, 1, p, 360, HOST | 4), "null out": (pt._h, 8, 1, None, 360, HOST), "null out, device": (pt._h, 8, 1, None, 360, 0),
             "one byte short": (pt._h, 8, 1, p, 359, HOST), "one byte long": (pt._h, 8, 1, p, 361, HOST), "RGBA8 size for RGB8": (pt._h, 8, 1, p, 480, HOST),
             "RGB8 size for RGBA8": (pt._h, 8, 2, p, 360, HOST), "RGB8 size for the mean": (pt._h, 8, 0, p, 360, HOST), "zero bytes": (pt._h, 8, 1, p, 0, HOST)}
    for what, args in cases.items():
        assert lib.amber_hip_pt_resolve(*args) == -1, what                                # AMBER_EINVAL
        assert b"amber_hip_pt_resolve" in lib.amber_hip_last_error(), what
        assert (buf == 0xAB).all(), what                                                   # no effect
    with pytest.raises(amber.AmberError):
        pt.resolve(8, 5)
    assert np.array_equal(pt.resolve(8, amber.RESOLVE_RGBA8), good)
    if amber.math_mode() == amber.MATH_GLIBC:
        assert np.array_equal(good[..., :3], O.tonemap(pt.download()[0] / F32(8)))
    pt.close()


# ---- 7: the product library --------------------------------------------------------------------------------------------------------------------
PRODUCT_CHILD = r"""
import os, sys, json
sys.path.insert(0, {root!r})
import numpy as np
import amber_amd as A
assert A.library_path().name == "libamber_hip.so" and not A.is_lab()
pt = A.PathTracer(A.HostScene.cornell_box(), A.Sensor.default(72, 48), seed=5)
pt.render_pass(0, 16)
total, _ = pt.download()
np.save(os.path.join({tmp!r}, "sum.npy"), total); np.save(os.path.join({tmp!r}, "rgb8.npy"), pt.resolve(16, A.RESOLVE_RGB8))
same_as_host = bool(np.array_equal(pt.resolve(16, A.RESOLVE_RGB8), A.tonemap(total / np.float32(16))))
pt.close()
print("RESULT " + json.dumps(dict(same_as_host=same_as_host, math=A.math_mode())))
"""


def test_product_library(amber, tmp_path):
    assert amber.is_lab()
    res = _child(PRODUCT_CHILD, env=dict(os.environ, AMBER_AMD_LIB="libamber_hip.so"), tmp=str(tmp_path))
    assert res["math"] == amber.MATH_GLIBC and res["same_as_host"]
    total, rgb = np.load(tmp_path / "sum.npy"), np.load(tmp_path / "rgb8.npy")
    assert total.shape == (48, 72, 3) and np.array_equal(rgb, O.tonemap(total / F32(16)))

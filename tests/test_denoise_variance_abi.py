"""Batch moments and amber_hip_pt_denoise_variance at the ABI level: the declarations and the two structs in include/amber_hip.h and their mirror in
amber_amd/api.py (no GPU), and on the GPU every AMBER_EINVAL the header names -- each with a message, no effect and the handle working afterwards --
a striped handle and the empty band."""
import ctypes
import inspect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import amber_amd as A
from amber_amd import api
import denoise_variance_reference as V
from test_moments import light_room

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "amber_hip.h").read_text()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
NAMES = ["amber_hip_pt_render_batch", "amber_hip_pt_moments_clear", "amber_hip_pt_moments_download", "amber_hip_pt_device_moments", "amber_hip_pt_denoise_variance"]
F32 = np.float32
EINVAL = -1


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- no GPU ------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    for decl in (r"int\s+amber_hip_pt_render_batch\(amber_hip_pt\*,\s*uint32_t first_sample,\s*uint32_t n_samples\);",
                 r"int\s+amber_hip_pt_moments_clear\(amber_hip_pt\*\);",
                 r"int\s+amber_hip_pt_moments_download\(amber_hip_pt\*,\s*AmberMomentsPixel\* out\);",
                 r"int\s+amber_hip_pt_device_moments\(amber_hip_pt\*,\s*void\*\* dptr,\s*uint64_t\* n_pixels\);",
                 r"int\s+amber_hip_pt_denoise_variance\(amber_hip_pt\*,\s*uint32_t n_samples,\s*const AmberDenoiseVarianceParams\* params,\s*uint32_t format,\s*void\* out,"
                 r"\s*uint64_t out_bytes,\s*uint32_t flags\s*\);"):
        assert re.search(decl, CODE), decl
    assert re.search(r"#define AMBER_HIP_ABI_VERSION 3\b", HEADER)                    # new functions only


def test_the_structs_have_the_given_sizes_and_orders():
    assert re.search(r"typedef struct \{\s*float m1, m2, batches, pad;\s*\} AmberMomentsPixel;", CODE)
    assert re.search(r"typedef struct \{\s*uint32_t levels;\s*float k_normal;\s*float k_albedo;\s*float k_depth;\s*float k_lum;\s*uint32_t var_radius;\s*uint32_t reserved\[2\];\s*\} "
                     r"AmberDenoiseVarianceParams;", CODE)
    M, P = api.MomentsPixel, api.DenoiseVarianceParams
    assert ctypes.sizeof(M) == 16 and A.MomentsPixel is M and [(n, t) for n, t in M._fields_] == [(n, ctypes.c_float) for n in ("m1", "m2", "batches", "pad")]
    assert ctypes.sizeof(P) == 32 and A.DenoiseVarianceParams is P
    assert [(n, ctypes.sizeof(t)) for n, t in P._fields_] == [("levels", 4), ("k_normal", 4), ("k_albedo", 4), ("k_depth", 4), ("k_lum", 4), ("var_radius", 4), ("reserved", 8)]
    assert (P.levels.offset, P.k_normal.offset, P.k_albedo.offset, P.k_depth.offset, P.k_lum.offset, P.var_radius.offset, P.reserved.offset) == (0, 4, 8, 12, 16, 20, 24)
    assert [t for _, t in P._fields_[:6]] == [ctypes.c_uint32] + [ctypes.c_float] * 4 + [ctypes.c_uint32]


def test_python_mirrors_them():
    for name in NAMES:
        assert name in api.ABI_SYMBOLS and name not in api.LAB_SYMBOLS
    for method in ("render_batch", "moments_clear", "moments_download", "device_moments", "denoise_variance"):
        assert callable(getattr(A.PathTracer, method, None)), method
    sig = inspect.signature(A.PathTracer.denoise_variance)
    assert list(sig.parameters) == ["self", "n_samples", "levels", "k_normal", "k_albedo", "k_depth", "k_lum", "var_radius", "format", "mirror", "out"]
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(levels=5, k_normal=4.0, k_albedo=100.0, k_depth=10.0, k_lum=16.0, var_radius=3, format=A.RESOLVE_RGB8, mirror=False, out=None)
    assert {k: defaults[k] for k in V.DEFAULTS} == V.DEFAULTS                          # the restatement's defaults are the binding's


def test_both_libraries_export_the_symbols(amber):
    lib_dir = ROOT / "amber_amd" / "lib"
    for lib in (api.PRODUCT_LIB, api.LAB_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", str(lib_dir / lib)], capture_output=True, text=True, check=True).stdout
        for name in NAMES:
            assert re.search(r" T " + name + r"$", out, re.M), (lib, name)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------
def cornell(amber, w=20, h=6, **kwargs):
    return amber.PathTracer(amber.HostScene.cornell_box(), amber.Sensor.default(w, h), **kwargs)


@pytest.mark.gpu
def test_moments_errors_are_einval_and_leave_the_handle_working(amber):
    lib = amber.load_library()
    pt, twin = cornell(amber, seed=1), cornell(amber, seed=1)
    pt.render_batch(0, 8)
    twin.render_batch(0, 8)
    buf = np.full(20 * 6 * 4, 7, F32)
    ptr, n = ctypes.c_void_p(), ctypes.c_uint64()
    cases = {"render_batch, null handle": (lib.amber_hip_pt_render_batch, (None, 0, 1)),
             "render_batch, sample index overflow": (lib.amber_hip_pt_render_batch, (pt._h, 0xffffffff, 1)),
             "render_batch, sample index overflow by a long batch": (lib.amber_hip_pt_render_batch, (pt._h, 2, 0xfffffffe)),
             "moments_clear, null handle": (lib.amber_hip_pt_moments_clear, (None,)),
             "moments_download, null handle": (lib.amber_hip_pt_moments_download, (None, buf.ctypes.data)),
             "moments_download, null out": (lib.amber_hip_pt_moments_download, (pt._h, None)),
             "device_moments, null handle": (lib.amber_hip_pt_device_moments, (None, ctypes.byref(ptr), ctypes.byref(n))),
             "device_moments, null dptr": (lib.amber_hip_pt_device_moments, (pt._h, None, ctypes.byref(n)))}
    for what, (entry, args) in cases.items():
        assert entry(*args) == EINVAL, what
        assert what.split(",")[0].encode() in lib.amber_hip_last_error(), what
        assert (buf == 7).all() and ptr.value is None, what
    assert lib.amber_hip_pt_render_pass(pt._h, 0xffffffff, 1) == EINVAL               # "as render_pass gives it"
    assert lib.amber_hip_pt_device_moments(pt._h, ctypes.byref(ptr), None) == 0 and ptr.value       # n_pixels may be NULL
    (got, got_rays), (want, want_rays) = pt.download(), twin.download()
    assert np.array_equal(bits(got), bits(want)) and got_rays == want_rays
    assert np.array_equal(bits(pt.moments_download()), bits(twin.moments_download())) and (pt.moments_download()[..., 2] == 1).all()
    pt.render_batch(8, 120)                                                             # and the handle renders afterwards
    twin.render_batch(8, 120)
    assert np.array_equal(bits(pt.download()[0]), bits(twin.download()[0])) and np.array_equal(bits(pt.moments_download()), bits(twin.moments_download()))
    assert (pt.moments_download()[..., 2] == 2).all()
    for p in (pt, twin):
        p.close()
    if amber.is_lab():                                                                  # the lab engine WAVEFRONT: refused, and its render_pass works on
        wf = cornell(amber, seed=1, engine=amber.ENGINE_WAVEFRONT)
        assert lib.amber_hip_pt_render_batch(wf._h, 0, 4) == EINVAL and b"WAVEFRONT" in lib.amber_hip_last_error()
        wf.render_pass(0, 8)
        plain = cornell(amber, seed=1)
        plain.render_pass(0, 8)
        assert np.array_equal(bits(wf.download()[0]), bits(plain.download()[0])) and not wf.moments_download().any()
        wf.close()
        plain.close()


@pytest.mark.gpu
def test_filter_errors_are_einval_and_leave_the_handle_working(amber):
    lib = amber.load_library()
    pt = cornell(amber, seed=1)
    for s in range(8):
        pt.render_batch(s, 1)
    pt.aov_pass(0, 8)
    good = pt.denoise_variance(8, format=amber.RESOLVE_RGBA8)
    HOST = amber.RESOLVE_HOST
    buf = np.full(20 * 6 * 12 + 64, 0xAB, np.uint8)
    p = buf.ctypes.data

    def P(**over):
        f = dict(V.DEFAULTS)
        reserved = over.pop("reserved", (0, 0))
        f.update(over)
        return ctypes.byref(amber.DenoiseVarianceParams(reserved=(ctypes.c_uint32 * 2)(*reserved), **f))
    cases = {"null handle": (None, 8, P(), 1, p, 360, HOST), "null params": (pt._h, 8, None, 1, p, 360, HOST), "n_samples == 0": (pt._h, 0, P(), 1, p, 360, HOST),
             "levels 0": (pt._h, 8, P(levels=0), 1, p, 360, HOST), "levels 9": (pt._h, 8, P(levels=9), 1, p, 360, HOST),
             "var_radius 4": (pt._h, 8, P(var_radius=4), 1, p, 360, HOST), "var_radius 2^32 - 1": (pt._h, 8, P(var_radius=0xffffffff), 1, p, 360, HOST),
             "unknown format": (pt._h, 8, P(), 3, p, 360, HOST), "unknown flag bits": (pt._h, 8, P(), 1, p, 360, HOST | 4),
             "null out": (pt._h, 8, P(), 1, None, 360, HOST), "null out, device": (pt._h, 8, P(), 1, None, 360, 0),
             "one byte short": (pt._h, 8, P(), 1, p, 359, HOST), "one byte long": (pt._h, 8, P(), 1, p, 361, HOST), "RGBA8 size for RGB8": (pt._h, 8, P(), 1, p, 480, HOST),
             "RGB8 size for RGBA8": (pt._h, 8, P(), 2, p, 360, HOST), "RGB8 size for the mean": (pt._h, 8, P(), 0, p, 360, HOST), "zero bytes": (pt._h, 8, P(), 1, p, 0, HOST),
             "a misaligned device pointer": (pt._h, 8, P(), 2, pt.device_framebuffer()[0] + 2, 480, 0)}
    for i in range(2):
        cases[f"reserved[{i}]"] = (pt._h, 8, P(reserved=[int(j == i) for j in range(2)]), 1, p, 360, HOST)
    for field in ("k_normal", "k_albedo", "k_depth", "k_lum"):
        for bad in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
            cases[f"{field} = {bad}"] = (pt._h, 8, P(**{field: bad}), 1, p, 360, HOST)
    before = pt.download()
    for what, args in cases.items():
        assert lib.amber_hip_pt_denoise_variance(*args) == EINVAL, what
        assert b"amber_hip_pt_denoise_variance" in lib.amber_hip_last_error(), what
        assert (buf == 0xAB).all(), what                                                   # no effect
    after = pt.download()
    assert np.array_equal(bits(before[0]), bits(after[0])) and before[1] == after[1]
    # amber_hip_pt_denoise keeps its own: a struct of the other filter with a word where its reserved[0] lies is refused by it
    plain = amber.DenoiseParams(levels=5, k_normal=4.0, k_albedo=100.0, k_depth=10.0, k_color=0.25, reserved=(ctypes.c_uint32 * 3)(3, 0, 0))
    assert lib.amber_hip_pt_denoise(pt._h, 8, ctypes.byref(plain), 1, p, 360, HOST) == EINVAL and (buf == 0xAB).all()
    with pytest.raises(amber.AmberError):
        pt.denoise_variance(8, format=5)
    with pytest.raises(amber.AmberError):
        pt.denoise_variance(8, var_radius=4)
    for ok in (dict(var_radius=0), dict(k_lum=0.0), dict(levels=8)):
        assert pt.denoise_variance(8, **ok).shape == (6, 20, 3)
    assert np.array_equal(pt.denoise_variance(8, format=amber.RESOLVE_RGBA8), good)
    pt.render_batch(8, 120)                                                                 # and the handle renders afterwards
    pt.aov_pass(8, 120)
    assert np.array_equal(bits(pt.denoise_variance(128, format=amber.RESOLVE_MEAN_F32)),
                          bits(V.denoise_variance(pt.download()[0], pt.aov_download(), pt.moments_download(), 128)))
    pt.close()


@pytest.mark.gpu
def test_a_striped_handle_and_the_empty_band(amber):
    lib = amber.load_library()
    room = amber.HostScene.create_arrays(**light_room())                               # (the Cornell box leaves eight rows of a 64-spp frame black)
    striped, twin = (amber.PathTracer(room, amber.Sensor.default(64, 48), seed=5, rows=(2, 24), stripe=(2, 6)) for _ in range(2))
    assert len(striped.row_index) == 8
    sums = []
    for first, n in ((0, 8), (8, 56)):                                                  # batches work on any band: the moments are per local pixel
        striped.render_batch(first, n)
        twin.clear()
        twin.render_pass(first, n)
        sums.append(twin.download()[0])
    moments = striped.moments_download()
    assert moments.shape == (8, 64, 4) and (moments[..., 2] == 2).all()
    assert np.array_equal(bits(moments), bits(V.moments_update(V.moments_update(np.zeros((8, 64, 4), F32), sums[0], 8), sums[1], 56)))
    assert np.array_equal(bits(striped.download()[0]), bits(sums[0] + sums[1])) and sums[1].any()
    buf = np.full(8 * 64 * 3, 0xAB, np.uint8)
    params = amber.DenoiseVarianceParams(**V.DEFAULTS)
    assert lib.amber_hip_pt_denoise_variance(striped._h, 64, ctypes.byref(params), amber.RESOLVE_RGB8, buf.ctypes.data, buf.nbytes, amber.RESOLVE_HOST) == EINVAL
    assert b"amber_hip_pt_denoise_variance" in lib.amber_hip_last_error() and b"strip" in lib.amber_hip_last_error() and (buf == 0xAB).all()
    with pytest.raises(amber.AmberError):
        striped.denoise_variance(64)
    assert striped.resolve(64).shape == (8, 64, 3)                                     # the handle works
    for pt in (striped, twin):
        pt.close()
    empty = amber.PathTracer(amber.HostScene.cornell_box(), amber.Sensor.default(64, 48), seed=5, rows=(5, 5))
    assert lib.amber_hip_pt_render_batch(empty._h, 0, 4) == 0 and lib.amber_hip_pt_moments_clear(empty._h) == 0
    for fmt in (0, 1, 2):
        assert lib.amber_hip_pt_denoise_variance(empty._h, 4, ctypes.byref(params), fmt, None, 0, 0) == 0
        assert lib.amber_hip_pt_denoise_variance(empty._h, 4, ctypes.byref(params), fmt, None, 0, amber.RESOLVE_HOST | amber.RESOLVE_MIRROR_X) == 0
    assert empty.denoise_variance(4).shape == (0, 64, 3) and empty.moments_download().shape == (0, 64, 4) and empty.device_moments() == (None, 0)
    assert lib.amber_hip_pt_denoise_variance(empty._h, 4, ctypes.byref(params), amber.RESOLVE_RGB8, None, 3, 0) == EINVAL     # the exact size holds for an empty band too
    empty.close()

"""ctypes binding of include/amber_hip.h and include/amber_host.h (no compute in Python)."""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

_ROOT = Path(__file__).resolve().parent
# AMBER_AMD_LIB selects another build next to the product library: libamber_hip_lab.so (tests/ and the tools that use the known-answer entry
# points, signatures or the measured-and-kept schedulers) or a measurement build (stamps, portable math); default = the product
_LIB_PATH = _ROOT / "lib" / os.environ.get("AMBER_AMD_LIB", "libamber_hip.so")
_lib = None


class AmberError(RuntimeError):
    """Raised for every non-zero return code of the C ABI (message = amber_hip_last_error())."""


# ---- plain-data structs (include/amber_hip.h) ---------------------------------------------------
class FlatObject(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("material", C.c_uint32), ("p", C.c_float * 12)]


class FlatMaterial(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("rho", C.c_float * 3), ("param", C.c_float), ("r0", C.c_float)]


class FlatThinLens(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("global_", C.c_float * 9), ("local_", C.c_float * 9),
                ("focus_distance", C.c_float), ("sensor_distance", C.c_float), ("p_area", C.c_float),
                ("n_blades", C.c_uint32), ("first_blade_object", C.c_uint32), ("kind", C.c_uint32)]


class FlatLight(C.Structure):
    _fields_ = [("object", C.c_uint32), ("cum_power", C.c_float), ("pdf_area", C.c_float), ("irradiance", C.c_float * 3)]


class FlatSceneC(C.Structure):
    _fields_ = [("objects", C.POINTER(FlatObject)), ("n_objects", C.c_uint32),
                ("materials", C.POINTER(FlatMaterial)), ("n_materials", C.c_uint32), ("lens", FlatThinLens),
                ("lights", C.POINTER(FlatLight)), ("n_lights", C.c_uint32)]


class Splat(C.Structure):
    _fields_ = [("path", C.c_uint32), ("sample", C.c_uint32), ("bounce", C.c_uint32), ("pixel", C.c_uint32),
                ("rgb", C.c_float * 3), ("pad", C.c_uint32)]


class Sensor(C.Structure):
    """rendering::Sensor(width, height, scene_width, scene_height) -- application.cc:89-94."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("scene_width", C.c_float), ("scene_height", C.c_float)]

    @classmethod
    def default(cls, width: int, height: int) -> "Sensor":
        # application.cc:89-94: Sensor(w, h, 0.036, 0.036 / w * h) -- doubles narrowed to real_type
        return cls(width, height, np.float32(0.036), np.float32(0.036 / width * height))


class PtParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("max_depth", C.c_uint32), ("device", C.c_int32), ("row_begin", C.c_uint32),
                ("row_end", C.c_uint32), ("stream", C.c_void_p), ("engine", C.c_uint32), ("stripe_rows", C.c_uint32),
                ("stripe_period", C.c_uint32), ("reserved", C.c_uint32)]


class BuildInfo(C.Structure):
    """AmberBuildInfo: engine BVH's tree as create built it (amber_hip_pt_build_info)."""
    _fields_ = [("where", C.c_uint32), ("fallback_reason", C.c_uint32), ("n_nodes", C.c_uint32), ("n_leaves", C.c_uint32), ("depth", C.c_uint32),
                ("pad", C.c_uint32), ("tree_ms", C.c_double), ("create_ms", C.c_double)]


class UpdateInfo(C.Structure):
    """AmberUpdateInfo: what amber_hip_pt_update_objects did, and the tree now in use."""
    _fields_ = [("mode_used", C.c_uint32), ("fallback_reason", C.c_uint32), ("n_nodes", C.c_uint32), ("depth", C.c_uint32),
                ("area_before", C.c_float), ("area_after", C.c_float), ("update_ms", C.c_double)]


class LtPassInfo(C.Structure):
    """AmberLtPassInfo: the totals of one amber_hip_lt_render_pass call -- 32 bytes."""
    _fields_ = [("n_splats", C.c_uint64), ("n_rays", C.c_uint64), ("n_launches", C.c_uint32), ("n_repeats", C.c_uint32),
                ("longest_run", C.c_uint32), ("pad", C.c_uint32)]


class Photon(C.Structure):
    """AmberPhoton: a light-path vertex -- pos, object | dir_out, path | weight, sample | normal, bounce: 64 bytes, four float4 (amber_hip_lt_trace_photons)."""
    _fields_ = [("pos", C.c_float * 3), ("object", C.c_int32), ("dir_out", C.c_float * 3), ("path", C.c_uint32),
                ("weight", C.c_float * 3), ("sample", C.c_uint32), ("normal", C.c_float * 3), ("bounce", C.c_uint32)]


class PhotonInfo(C.Structure):
    """AmberPhotonInfo: the totals of one amber_hip_lt_trace_photons call -- 32 bytes."""
    _fields_ = [("n_photons", C.c_uint64), ("n_written", C.c_uint64), ("n_rays", C.c_uint64), ("n_launches", C.c_uint32), ("n_repeats", C.c_uint32)]


class AccumulateInfo(C.Structure):
    """AmberAccumulateInfo (lab build): what one amber_hip_kat_accumulate call did."""
    _fields_ = [("n_launches", C.c_uint32), ("n_repeats", C.c_uint32), ("rec_count", C.c_uint32), ("flag_words_set", C.c_uint32),
                ("flags_dirty", C.c_uint32)]


LT_SPLAT_CAPACITY0 = 65536   # AMBER_LT_SPLAT_CAPACITY0: records the handle's splat buffer holds before the first growth
SPLAT_DTYPE = np.dtype([("path", np.uint32), ("sample", np.uint32), ("bounce", np.uint32), ("pixel", np.uint32), ("rgb", np.float32, (3,)), ("pad", np.uint32)])   # AmberSplat
PHOTON_DIFFUSE, PHOTON_SPECULAR, PHOTON_LIGHT, PHOTON_EYE, PHOTON_ALL = 1, 2, 4, 8, 15   # AMBER_PHOTON_*: the surface kinds whose vertices are recorded
PHOTONS_HOST = 1             # AMBER_PHOTONS_HOST: out is a host pointer
PHOTON_CAPACITY0 = 65536     # AMBER_PHOTON_CAPACITY0: records the handle's photon staging buffer holds before the first growth
PHOTON_DTYPE = np.dtype([("pos", np.float32, (3,)), ("object", np.int32), ("dir_out", np.float32, (3,)), ("path", np.uint32),
                         ("weight", np.float32, (3,)), ("sample", np.uint32), ("normal", np.float32, (3,)), ("bounce", np.uint32)])   # AmberPhoton
PM_RAW_SUM = 2               # AMBER_PM_RAW_SUM: amber_hip_pm_gather returns the plain sum S instead of (S * kern) * weight
GATHER_QUERY_DTYPE = np.dtype([("pos", np.float32, (3,)), ("radius", np.float32), ("normal", np.float32, (3,)), ("object", np.int32),
                               ("dir_out", np.float32, (3,)), ("pad0", np.uint32), ("weight", np.float32, (3,)), ("pad1", np.uint32)])   # AmberGatherQuery
GATHER_RESULT_DTYPE = np.dtype([("rgb", np.float32, (3,)), ("n_used", np.uint32), ("r2_used", np.float32), ("n_in_radius", np.uint32),
                                ("pad", np.uint32, (2,))])                                                                                   # AmberGatherResult


class PhotonMapInfo(C.Structure):
    """AmberPhotonMapInfo: what amber_hip_pm_build made -- counts, the grid (dims, the cell size used and how often it doubled, bounds), the largest cell,
    the host's wall-clock milliseconds: 72 bytes."""
    _fields_ = [("n_photons", C.c_uint64), ("n_dropped", C.c_uint64), ("dims", C.c_uint32 * 3), ("n_doublings", C.c_uint32), ("cell_size", C.c_float),
                ("lo", C.c_float * 3), ("hi", C.c_float * 3), ("max_cell_count", C.c_uint32), ("build_ms", C.c_double)]


class Ray(C.Structure):
    """AmberRay: origin, t_max, dir, pad -- 32 bytes (amber_hip_pt_cast_rays / amber_hip_pt_occluded)."""
    _fields_ = [("origin", C.c_float * 3), ("t_max", C.c_float), ("dir", C.c_float * 3), ("pad", C.c_uint32)]


class RayHit(C.Structure):
    """AmberRayHit: t (NaN = miss), object (scene index, -1 = miss), pos, normal -- 32 bytes."""
    _fields_ = [("t", C.c_float), ("object", C.c_int32), ("pos", C.c_float * 3), ("normal", C.c_float * 3)]


class PathRay(C.Structure):
    """AmberPathRay: origin, dir, weight (each padded to 16 bytes), rng_state, pad -- 64 bytes (amber_hip_pt_trace_paths)."""
    _fields_ = [("origin", C.c_float * 3), ("pad0", C.c_uint32), ("dir", C.c_float * 3), ("pad1", C.c_uint32),
                ("weight", C.c_float * 3), ("pad2", C.c_uint32), ("rng_state", C.c_uint64), ("pad3", C.c_uint64)]


class PathResult(C.Structure):
    """AmberPathResult: the sum of the samples' measurements, the casts, the sampler state after the last sample -- 32 bytes."""
    _fields_ = [("rgb", C.c_float * 3), ("casts", C.c_uint32), ("rng_state", C.c_uint64), ("pad", C.c_uint32 * 2)]


class AovPixel(C.Structure):
    """AmberAovPixel: the sums of albedo, depth, normal and coverage of a pixel's first hits -- 32 bytes (amber_hip_pt_aov_pass)."""
    _fields_ = [("albedo", C.c_float * 3), ("depth", C.c_float), ("normal", C.c_float * 3), ("coverage", C.c_float)]


class DenoiseParams(C.Structure):
    """AmberDenoiseParams: levels (1..8) and the four edge-stopping constants of amber_hip_pt_denoise -- 32 bytes."""
    _fields_ = [("levels", C.c_uint32), ("k_normal", C.c_float), ("k_albedo", C.c_float), ("k_depth", C.c_float), ("k_color", C.c_float),
                ("reserved", C.c_uint32 * 3)]


class MomentsPixel(C.Structure):
    """AmberMomentsPixel: the sums of the batches' luminance and of its square, and the number of batches -- 16 bytes (amber_hip_pt_render_batch)."""
    _fields_ = [("m1", C.c_float), ("m2", C.c_float), ("batches", C.c_float), ("pad", C.c_float)]


class DenoiseVarianceParams(C.Structure):
    """AmberDenoiseVarianceParams: levels (1..8), the three guide stops' constants, k_lum and var_radius (0..3) of amber_hip_pt_denoise_variance -- 32 bytes."""
    _fields_ = [("levels", C.c_uint32), ("k_normal", C.c_float), ("k_albedo", C.c_float), ("k_depth", C.c_float), ("k_lum", C.c_float),
                ("var_radius", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class TemporalParams(C.Structure):
    """AmberTemporalParams: levels (0..8), max_history (1..65535) and the four edge-stopping constants of amber_hip_pt_temporal -- 32 bytes."""
    _fields_ = [("levels", C.c_uint32), ("max_history", C.c_uint32), ("k_normal", C.c_float), ("k_albedo", C.c_float), ("k_depth", C.c_float),
                ("k_color", C.c_float), ("reserved", C.c_uint32 * 2)]


class HistoryPixel(C.Structure):
    """AmberHistoryPixel: the accumulated colour, the history length and the two running moments of the luminance -- 32 bytes (amber_hip_pt_temporal)."""
    _fields_ = [("color", C.c_float * 3), ("length", C.c_float), ("m1", C.c_float), ("m2", C.c_float), ("pad", C.c_float * 2)]


class BvhDumpInfo(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("n_prims", C.c_uint32), ("root", C.c_int32), ("depth", C.c_uint32),
                ("gmin", C.c_float * 3), ("step", C.c_float * 3), ("reach", C.c_float * 3)]


class HostStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("passes", C.c_uint64), ("launches", C.c_uint32), ("pad", C.c_uint32), ("kernel_ms", C.c_double)]


PRIM_TRIANGLE, PRIM_SPHERE, PRIM_DISK, PRIM_CYLINDER = 0, 1, 2, 3
_RECORD = np.dtype([("kind", np.uint32), ("material", np.uint32), ("p", np.float32, (12,))])     # AmberFlatObject
MAT_LAMBERTIAN, MAT_PHONG, MAT_SPECULAR, MAT_REFRACTION, MAT_DIFFUSE_LIGHT, MAT_EYE = 0, 1, 2, 3, 4, 5
ENGINE_AUTO, ENGINE_LIST, ENGINE_TWO_PHASE, ENGINE_BVH, ENGINE_WAVEFRONT = 0, 1, 2, 3, 4
ENGINE_REFERENCE_BVH = 6     # the reference's own tree and traversal order: every ray gets the hit the reference's BVH gives it (include/amber_hip.h)
PT_FLAG_NULL_STREAM, PT_FLAG_BVH_POOL, PT_FLAG_BVH_ITEMS = 1, 2, 4
PT_FLAG_DEVICE_BUILD = 8     # engine BVH: create builds the tree on the device (include/amber_hip.h)
PT_FLAG_NO_SCOUT = 16        # the 32-object two-phase engine: every path carries its weight (no scout + replay); same bits (include/amber_hip.h)
BUILD_NONE, BUILD_HOST, BUILD_DEVICE, BUILD_HOST_FALLBACK = 0, 1, 2, 3
BUILD_REASON_NONE, BUILD_REASON_DEPTH, BUILD_REASON_WIDE, BUILD_REASON_BOUNDS = 0, 1, 2, 3
RAYS_HOST = 1                # amber_hip_pt_cast_rays / amber_hip_pt_occluded: rays and output are host pointers
_RAY = np.dtype([("origin", np.float32, (3,)), ("t_max", np.float32), ("dir", np.float32, (3,)), ("pad", np.uint32)])       # AmberRay
_RAY_HIT = np.dtype([("t", np.float32), ("object", np.int32), ("pos", np.float32, (3,)), ("normal", np.float32, (3,))])    # AmberRayHit
_PATH_RAY = np.dtype([("origin", np.float32, (3,)), ("pad0", np.uint32), ("dir", np.float32, (3,)), ("pad1", np.uint32),
                      ("weight", np.float32, (3,)), ("pad2", np.uint32), ("rng_state", np.uint64), ("pad3", np.uint64)])                 # AmberPathRay
_PATH_RESULT = np.dtype([("rgb", np.float32, (3,)), ("casts", np.uint32), ("rng_state", np.uint64), ("pad", np.uint32, (2,))])          # AmberPathResult
RESOLVE_MEAN_F32, RESOLVE_RGB8, RESOLVE_RGBA8 = 0, 1, 2     # amber_hip_pt_resolve: format
RESOLVE_HOST, RESOLVE_MIRROR_X = 1, 2                        # ... and flags: out is a host pointer / columns written right to left
UPDATE_REFIT, UPDATE_REBUILD = 0, 1     # amber_hip_pt_update_objects: keep the tree's topology and recompute its boxes / build the Morton tree again

# every symbol include/amber_hip.h and include/amber_host.h declare: what libamber_hip.so (the product) exports
ABI_SYMBOLS = [
    "amber_hip_pt_create", "amber_hip_pt_render_pass", "amber_hip_pt_clear", "amber_hip_pt_sync",
    "amber_hip_pt_download", "amber_hip_pt_device_framebuffer", "amber_hip_pt_stream", "amber_hip_pt_local_rows", "amber_hip_pt_kernel_time", "amber_hip_pt_build_info", "amber_hip_pt_update_objects", "amber_hip_pt_update_lens",
    "amber_hip_pt_cast_rays", "amber_hip_pt_occluded", "amber_hip_pt_resolve", "amber_hip_pt_destroy",
    "amber_hip_pt_trace_paths", "amber_hip_sampler_state",
    "amber_hip_pt_aov_pass", "amber_hip_pt_aov_clear", "amber_hip_pt_aov_download", "amber_hip_pt_device_aov", "amber_hip_pt_denoise",
    "amber_hip_pt_render_batch", "amber_hip_pt_moments_clear", "amber_hip_pt_moments_download", "amber_hip_pt_device_moments", "amber_hip_pt_denoise_variance",
    "amber_hip_pt_temporal", "amber_hip_pt_temporal_reset", "amber_hip_pt_history_download", "amber_hip_pt_device_history",
    "amber_hip_last_error", "amber_hip_abi_version", "amber_hip_math_mode", "amber_hip_device_count", "amber_hip_lt_trace", "amber_hip_lt_trace_range", "amber_hip_lt_render_pass",
    "amber_hip_lt_trace_photons", "amber_hip_pm_build", "amber_hip_pm_gather", "amber_hip_pm_release",
    "amber_host_cornell_box", "amber_host_scene_import", "amber_host_scene_create", "amber_host_scene_destroy", "amber_host_scene_flatten",
    "amber_host_pt_create", "amber_host_render", "amber_host_render_devices", "amber_host_last_error", "amber_host_tonemap", "amber_host_export",
]
# what include/amber_hip_lab.h declares: libamber_hip_lab.so (the same sources with -DAMBER_LAB) exports these as well
LAB_SYMBOLS = [
    "amber_hip_kat_cast", "amber_hip_kat_sample", "amber_hip_kat_eye", "amber_hip_kat_trace", "amber_hip_kat_math", "amber_hip_kat_signatures", "amber_hip_pt_signatures",
    "amber_hip_kat_traversal_rate", "amber_hip_kat_pixel_masks", "amber_hip_kat_bvh_dump", "amber_hip_kat_division",
    "amber_hip_kat_sqrt", "amber_hip_kat_sqrt_sweep", "amber_hip_kat_lt_accumulate", "amber_hip_kat_lt_stage_ms",
    "amber_hip_kat_photon_stage_ms", "amber_hip_kat_pm_stage_ms", "amber_hip_kat_bsdf",
    "amber_hip_kat_light_ray", "amber_hip_kat_lens_response", "amber_hip_kat_radiance", "amber_host_kat_scene_lights",
    "amber_hip_kat_accumulate", "amber_hip_kat_phase_a", "amber_hip_kat_scout_flags",
]
PRODUCT_LIB, LAB_LIB = "libamber_hip.so", "libamber_hip_lab.so"


def library_path() -> Path:
    return _LIB_PATH


def build_library(force: bool = False) -> Path:
    """Compile the HIP extension for gfx950 in-tree (hipcc cross-compiles without a GPU).  make is incremental, so it
    always runs where a compiler exists: an edited .hip/.h can never be tested against a stale library.  A box
    without hipcc uses the prebuilt library that travelled with the tree."""
    import shutil
    if shutil.which(os.environ.get("HIPCC", "hipcc")) or not _LIB_PATH.exists():
        subprocess.run(["make", "-C", str(_ROOT / "csrc")] + (["-B"] if force else []), check=True)
    return _LIB_PATH


def is_lab() -> bool:
    """True when the loaded library is a lab build (it has the entry points of include/amber_hip_lab.h)."""
    return hasattr(load_library(), "amber_hip_kat_cast")


def load_library() -> C.CDLL:
    """Load libamber_hip.so (or the build AMBER_AMD_LIB names).  Fails loudly: there is no CPU implementation to fall back to."""
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB_PATH.exists():
        raise AmberError(f"{_LIB_PATH} is missing: build it with `make -C amber_amd/csrc` "
                         "(or __graft_entry__.build()); amber_amd has no CPU fallback")
    lib = C.CDLL(str(_LIB_PATH))
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32
    lib.amber_hip_last_error.restype = C.c_char_p
    lib.amber_host_last_error.restype = C.c_char_p
    lib.amber_hip_pt_create.argtypes = [C.POINTER(FlatSceneC), C.POINTER(Sensor), C.POINTER(PtParams), C.POINTER(vp)]
    lib.amber_hip_pt_render_pass.argtypes = [vp, u32, u32]
    lib.amber_hip_pt_clear.argtypes = [vp]
    lib.amber_hip_pt_sync.argtypes = [vp]
    lib.amber_hip_pt_download.argtypes = [vp, vp, C.POINTER(u64)]
    lib.amber_hip_pt_device_framebuffer.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    lib.amber_hip_pt_local_rows.argtypes = [vp, C.POINTER(u32)]
    lib.amber_hip_pt_stream.argtypes = [vp, C.POINTER(vp)]
    lib.amber_hip_pt_kernel_time.argtypes = [vp, C.POINTER(u32), C.POINTER(C.c_double)]
    lib.amber_hip_pt_destroy.argtypes = [vp]
    lib.amber_hip_pt_destroy.restype = None
    if hasattr(lib, "amber_hip_pt_build_info"):    # absent only in older builds loaded by tools/ab_lib.py
        lib.amber_hip_pt_build_info.argtypes = [vp, C.POINTER(BuildInfo)]
    if hasattr(lib, "amber_hip_pt_update_objects"):
        lib.amber_hip_pt_update_objects.argtypes = [vp, u32, u32, vp, u32, C.POINTER(UpdateInfo)]
    if hasattr(lib, "amber_hip_pt_update_lens"):
        lib.amber_hip_pt_update_lens.argtypes = [vp, C.POINTER(FlatThinLens), vp, u32, C.POINTER(UpdateInfo)]
    if hasattr(lib, "amber_hip_pt_cast_rays"):
        lib.amber_hip_pt_cast_rays.argtypes = [vp, u64, vp, vp, u32]
        lib.amber_hip_pt_occluded.argtypes = [vp, u64, vp, vp, u32]
    if hasattr(lib, "amber_hip_pt_trace_paths"):
        lib.amber_hip_pt_trace_paths.argtypes = [vp, u64, vp, vp, u32, u32, u32]
        lib.amber_hip_sampler_state.argtypes = [u64, u32, u32]
        lib.amber_hip_sampler_state.restype = u64
    if hasattr(lib, "amber_hip_pt_resolve"):
        lib.amber_hip_pt_resolve.argtypes = [vp, u32, u32, vp, u64, u32]
    if hasattr(lib, "amber_hip_pt_aov_pass"):
        lib.amber_hip_pt_aov_pass.argtypes = [vp, u32, u32]
        lib.amber_hip_pt_aov_clear.argtypes = [vp]
        lib.amber_hip_pt_aov_download.argtypes = [vp, vp]
        lib.amber_hip_pt_device_aov.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    if hasattr(lib, "amber_hip_pt_denoise"):
        lib.amber_hip_pt_denoise.argtypes = [vp, u32, C.POINTER(DenoiseParams), u32, vp, u64, u32]
    if hasattr(lib, "amber_hip_pt_render_batch"):
        lib.amber_hip_pt_render_batch.argtypes = [vp, u32, u32]
        lib.amber_hip_pt_moments_clear.argtypes = [vp]
        lib.amber_hip_pt_moments_download.argtypes = [vp, vp]
        lib.amber_hip_pt_device_moments.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
        lib.amber_hip_pt_denoise_variance.argtypes = [vp, u32, C.POINTER(DenoiseVarianceParams), u32, vp, u64, u32]
    if hasattr(lib, "amber_hip_pt_temporal"):
        lib.amber_hip_pt_temporal.argtypes = [vp, u32, C.POINTER(TemporalParams), u32, vp, u64, u32]
        lib.amber_hip_pt_temporal_reset.argtypes = [vp]
        lib.amber_hip_pt_history_download.argtypes = [vp, vp]
        lib.amber_hip_pt_device_history.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    if hasattr(lib, "amber_hip_lt_trace"):     # absent only in older builds loaded by tools/ab_lib.py
        lib.amber_hip_lt_trace.argtypes = [vp, u32, u32, vp, u32, C.POINTER(u32), C.POINTER(u64)]
    if hasattr(lib, "amber_hip_lt_trace_range"):
        lib.amber_hip_lt_trace_range.argtypes = [vp, u32, u32, u32, u32, vp, u32, C.POINTER(u32), C.POINTER(u64)]
    if hasattr(lib, "amber_hip_lt_render_pass"):
        lib.amber_hip_lt_render_pass.argtypes = [vp, u32, u32, C.POINTER(LtPassInfo)]
        if hasattr(lib, "amber_hip_lt_trace_photons"):      # (a library built before it has no such symbol)
            lib.amber_hip_lt_trace_photons.argtypes = [vp, u32, u32, u32, u32, u32, vp, u64, C.POINTER(PhotonInfo), u32]
        if hasattr(lib, "amber_hip_kat_photon_stage_ms"):   # lab build
            lib.amber_hip_kat_photon_stage_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    if hasattr(lib, "amber_hip_pm_build"):             # (a library built before the photon map has no such symbols)
        lib.amber_hip_pm_build.argtypes = [vp, vp, u64, C.c_float, u32, C.POINTER(PhotonMapInfo)]
        lib.amber_hip_pm_gather.argtypes = [vp, u64, vp, vp, u32, u32]
        lib.amber_hip_pm_release.argtypes = [vp]
    if hasattr(lib, "amber_hip_kat_pm_stage_ms"):      # lab build
        lib.amber_hip_kat_pm_stage_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        lib.amber_hip_kat_bsdf.argtypes = [vp, u32, vp, vp, vp, vp, vp]
    if hasattr(lib, "amber_hip_kat_cast"):         # the lab build (include/amber_hip_lab.h); the product exports none of these
        if hasattr(lib, "amber_hip_kat_phase_a"):      # (a library built before it has no such symbol)
            lib.amber_hip_kat_phase_a.argtypes = [vp, u32, vp, vp, i32, vp, u64, C.POINTER(C.c_uint32)]
        lib.amber_hip_kat_cast.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp]
        lib.amber_hip_kat_sample.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp]
        lib.amber_hip_kat_eye.argtypes = [vp, u32, vp, vp, vp]
        lib.amber_hip_kat_trace.argtypes = [vp, u32, vp, vp, u32, vp, vp]
        lib.amber_hip_kat_math.argtypes = [i32, i32, u32, vp, vp]
        lib.amber_hip_kat_signatures.argtypes = [vp, u32, u32, vp]
        lib.amber_hip_kat_pixel_masks.argtypes = [vp, vp, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
        lib.amber_hip_kat_traversal_rate.argtypes = [vp, u32, vp, vp, u32, u32, u32, vp, vp, C.POINTER(C.c_double), vp]
        lib.amber_hip_pt_signatures.argtypes = [vp, u32, u32, vp]
        lib.amber_hip_kat_bvh_dump.argtypes = [vp, vp, u32, vp, u32, C.POINTER(BvhDumpInfo)]
        if hasattr(lib, "amber_hip_kat_division"):     # absent only in older builds loaded by tools/ab_lib.py
            lib.amber_hip_kat_division.argtypes = [i32, i32, u32, vp, vp]
        if hasattr(lib, "amber_hip_kat_sqrt"):         # the same
            lib.amber_hip_kat_sqrt.argtypes = [i32, i32, u32, vp, vp]
            lib.amber_hip_kat_sqrt_sweep.argtypes = [i32, u32, u64, C.POINTER(SqrtSweep)]
        if hasattr(lib, "amber_hip_kat_lt_accumulate"):    # the same
            lib.amber_hip_kat_lt_accumulate.argtypes = [vp, vp, u32]
            lib.amber_hip_kat_lt_stage_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        if hasattr(lib, "amber_hip_kat_light_ray"):        # the same
            lib.amber_hip_kat_light_ray.argtypes = [vp, u32, vp, vp, vp, vp, vp]
            lib.amber_hip_kat_lens_response.argtypes = [vp, u32, vp, vp, vp, vp, vp]
            lib.amber_hip_kat_radiance.argtypes = [vp, u32, vp, vp, vp, vp]
            lib.amber_host_kat_scene_lights.argtypes = [vp, C.POINTER(FlatLight), C.POINTER(u32)]
        if hasattr(lib, "amber_hip_kat_scout_flags"):      # (a measurement build of an older tree may lack it)
            lib.amber_hip_kat_scout_flags.argtypes = [vp, u32, u32, vp, u64, C.POINTER(u32), C.POINTER(u32)]
        if hasattr(lib, "amber_hip_kat_accumulate"):       # the same
            lib.amber_hip_kat_accumulate.argtypes = [vp, u32, vp, vp, u32, u32, u32, u64, C.POINTER(AccumulateInfo)]
    lib.amber_host_cornell_box.restype = vp
    lib.amber_host_cornell_box.argtypes = [C.c_float, C.c_float, u32]
    lib.amber_host_scene_import.restype = vp
    lib.amber_host_scene_import.argtypes = [C.c_char_p]
    lib.amber_host_scene_create.restype = vp
    lib.amber_host_scene_create.argtypes = [C.POINTER(FlatObject), u32, C.POINTER(FlatMaterial), u32, C.POINTER(C.c_float),
                                            C.c_float, C.c_float, C.c_float, u32, C.c_int]   # n_blades == 0 selects the pinhole lens
    lib.amber_host_scene_destroy.argtypes = [vp]
    lib.amber_host_scene_destroy.restype = None
    lib.amber_host_scene_flatten.argtypes = [vp, C.POINTER(FlatObject), C.POINTER(u32), C.POINTER(FlatMaterial), C.POINTER(u32),
                                             C.POINTER(FlatThinLens)]
    lib.amber_host_pt_create.argtypes = [vp, C.POINTER(Sensor), C.POINTER(PtParams), C.POINTER(vp)]
    lib.amber_host_render.argtypes = [vp, C.c_char_p, C.POINTER(Sensor), u32, u64, u32, C.c_int, u32, vp, C.POINTER(HostStats)]
    lib.amber_host_render_devices.argtypes = [vp, C.c_char_p, C.POINTER(Sensor), u32, u64, u32, C.POINTER(C.c_int), u32, u32, vp, C.POINTER(HostStats)]
    lib.amber_host_tonemap.argtypes = [vp, u32, u32, vp]
    lib.amber_host_export.argtypes = [vp, u32, u32, C.c_char_p, C.c_char_p]
    _lib = lib
    return lib


def _check(rc: int, host: bool = False) -> None:
    if rc != 0:
        lib = load_library()
        msg = (lib.amber_host_last_error() if host else lib.amber_hip_last_error()) or b""
        if host and not msg:
            msg = lib.amber_hip_last_error() or b""
        raise AmberError(f"amber error {rc}: {msg.decode(errors='replace')}")


def device_count() -> int:
    return int(load_library().amber_hip_device_count())


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


class HostScene:
    """Handle of a scene built by the C++ host object model (amber::scene::Scene)."""

    def __init__(self, handle):
        if not handle:
            raise AmberError("scene creation failed: " + (load_library().amber_host_last_error() or b"").decode())
        self._h = C.c_void_p(handle)

    @classmethod
    def cornell_box(cls, focal_length: float = 0.050, aperture_radius: float = 0.050, n_blades: int = 6) -> "HostScene":
        """etude::CornelBox(0.050, 0.050, 6) -- application.cc:68-73."""
        return cls(load_library().amber_host_cornell_box(focal_length, aperture_radius, n_blades))

    @classmethod
    def import_file(cls, filename) -> "HostScene":
        """cli::ImportScene(filename) + Scene::Create<BVH> (import.cc:49-167, application.cc:74-86); OBJ + MTL subset."""
        return cls(load_library().amber_host_scene_import(str(filename).encode()))

    @classmethod
    def create(cls, objects, materials, transform, focal_length, focus_distance, radius, n_blades, accel: int = 0) -> "HostScene":
        """objects: list of (kind, material, params...) ; materials: list of (kind, (r,g,b), param)."""
        objs = (FlatObject * max(1, len(objects)))()
        for i, (kind, mat, params) in enumerate(objects):
            objs[i].kind, objs[i].material = kind, mat
            for j, v in enumerate(params):
                objs[i].p[j] = v
        mats = (FlatMaterial * max(1, len(materials)))()
        for i, (kind, rho, param) in enumerate(materials):
            mats[i].kind, mats[i].param = kind, param
            for j in range(3):
                mats[i].rho[j] = rho[j]
        t = (C.c_float * 16)(*[float(x) for x in transform])
        return cls(load_library().amber_host_scene_create(objs, len(objects), mats, len(materials), t, focal_length,
                                                          focus_distance, radius, n_blades, accel))

    @classmethod
    def create_arrays(cls, kinds, material_index, params, materials, transform, focal_length, focus_distance, radius, n_blades,
                      accel: int = 0) -> "HostScene":
        """Bulk form of create(): kinds (n,) u32, material_index (n,) u32, params (n,12) f32 as numpy arrays."""
        n = len(kinds)
        dt = np.dtype([("kind", np.uint32), ("material", np.uint32), ("p", np.float32, (12,))])
        arr = np.zeros(n, dt)
        arr["kind"], arr["material"] = kinds, material_index
        arr["p"][:, : np.asarray(params).shape[1]] = params
        assert arr.itemsize == C.sizeof(FlatObject)
        mats = (FlatMaterial * max(1, len(materials)))()
        for i, (kind, rho, param) in enumerate(materials):
            mats[i].kind, mats[i].param = kind, param
            for j in range(3):
                mats[i].rho[j] = rho[j]
        t = (C.c_float * 16)(*[float(x) for x in transform])
        return cls(load_library().amber_host_scene_create(arr.ctypes.data_as(C.POINTER(FlatObject)), n, mats, len(materials), t,
                                                          focal_length, focus_distance, radius, n_blades, accel))

    def flatten(self):
        lib = load_library()
        no, nm = C.c_uint32(0), C.c_uint32(0)
        _check(lib.amber_host_scene_flatten(self._h, None, C.byref(no), None, C.byref(nm), None), host=True)
        objs, mats, lens = (FlatObject * no.value)(), (FlatMaterial * nm.value)(), FlatThinLens()
        _check(lib.amber_host_scene_flatten(self._h, objs, C.byref(no), mats, C.byref(nm), C.byref(lens)), host=True)
        return objs, mats, lens

    def lights(self):
        """Lab build: the light table flatten() computes for amber_hip_pt_create (FlatLight records in the light set's order)."""
        lib = load_library()
        n = C.c_uint32(0)
        _check(lib.amber_host_kat_scene_lights(self._h, None, C.byref(n)), host=True)
        out = (FlatLight * max(1, n.value))()
        _check(lib.amber_host_kat_scene_lights(self._h, out, C.byref(n)), host=True)
        return list(out[:n.value])

    def render(self, sensor: Sensor, spp: int, seed: int = 12345, max_depth: int = 0, device: int = 0,
               samples_per_launch: int = 0, algorithm: str = "pt", devices=None):
        """Algorithm<RGB>::Render through cli::MakeAlgorithm(algorithm) and cli::Context(1, spp).
        devices: list of HIP ordinals -> one engine handle per entry inside the one Render() call (HipPathTracingOptions.devices)."""
        out = np.empty((sensor.height, sensor.width, 3), np.float32)
        st = HostStats()
        devs = list(devices) if devices else [device]
        arr = (C.c_int * len(devs))(*devs)
        _check(load_library().amber_host_render_devices(self._h, algorithm.encode(), C.byref(sensor), spp, seed, max_depth, arr, len(devs),
                                                        samples_per_launch, out.ctypes.data, C.byref(st)), host=True)
        return out, {"rays": st.rays, "passes": st.passes, "launches": st.launches, "kernel_ms": st.kernel_ms}

    def close(self):
        if self._h:
            load_library().amber_host_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sampler_state(seed: int, pixel: int, sample: int) -> int:
    """amber_hip_sampler_state: the state the render kernels' sampler starts (pixel, sample) with under `seed` -- XorShiftSeed(SplitMix64(seed), pixel,
    sample), never 0.  The eye-ray generator then draws 5 times (thin lens) or twice (pinhole) before the first cast.  No device is touched."""
    return int(load_library().amber_hip_sampler_state(seed & 0xffffffffffffffff, pixel, sample))


def _splitmix64(z):
    """SplitMix64 on a numpy uint64 array (wrapping arithmetic)"""
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def sampler_states(seed: int, pixels, samples) -> np.ndarray:
    """sampler_state for arrays of pixels and samples at once: (n,) uint64, equal to amber_hip_sampler_state element by element."""
    pixels, samples = np.asarray(pixels, np.uint64), np.asarray(samples, np.uint64)
    hashed = _splitmix64(np.array([seed & 0xffffffffffffffff], np.uint64))[0]
    s = _splitmix64(hashed ^ ((pixels << np.uint64(32)) | samples))
    return np.where(s == 0, np.uint64(0x9E3779B97F4A7C15), s).astype(np.uint64)


class PathTracer:
    """amber_hip_pt handle: the device-side engine for one band of the framebuffer on one GPU."""

    def __init__(self, scene: HostScene, sensor: Sensor, seed: int = 12345, max_depth: int = 0, device: int = 0,
                 rows=None, stream: int | None = None, engine: int = ENGINE_AUTO, stripe=None, flags: int = 0):
        """rows = (y0, y1) contiguous band; stripe = (S, period) keeps only rows with (y - y0) % period < S;
        flags = AMBER_PT_FLAG_* bits (PT_FLAG_BVH_POOL: engine BVH with the per-wave ray pool scheduler; PT_FLAG_DEVICE_BUILD: engine BVH's tree
        built on the device at create)."""
        self.sensor, self.seed = sensor, seed
        self._scene, self._resident = scene, None     # update_objects: the scene's flattened kinds and materials (an update never changes them)
        rb, re = rows if rows is not None else (0, sensor.height)
        s_rows, s_period = stripe if stripe else (0, 0)
        p = PtParams(seed, max_depth, device, rb, re, stream, engine, s_rows, s_period, flags)
        h = C.c_void_p()
        _check(load_library().amber_host_pt_create(scene._h, C.byref(sensor), C.byref(p), C.byref(h)), host=True)
        self._h = h
        ys = np.arange(rb, re)
        self.row_index = ys[(ys - rb) % s_period < s_rows] if s_rows else ys   # global row of every local row
        n = C.c_uint32()
        _check(load_library().amber_hip_pt_local_rows(self._h, C.byref(n)))
        assert n.value == len(self.row_index)
        self.rows = (rb, re)

    @property
    def band_shape(self):
        return (len(self.row_index), self.sensor.width, 3)

    def render_pass(self, first_sample: int, n_samples: int) -> None:
        _check(load_library().amber_hip_pt_render_pass(self._h, first_sample, n_samples))

    def clear(self) -> None:
        _check(load_library().amber_hip_pt_clear(self._h))

    def sync(self) -> None:
        _check(load_library().amber_hip_pt_sync(self._h))

    def download(self):
        out = np.empty(self.band_shape, np.float32)
        rays = C.c_uint64()
        _check(load_library().amber_hip_pt_download(self._h, out.ctypes.data, C.byref(rays)))
        return out, rays.value

    def ray_count(self) -> int:
        rays = C.c_uint64()
        _check(load_library().amber_hip_pt_download(self._h, None, C.byref(rays)))
        return rays.value

    def stream(self) -> int:
        """hipStream_t (as an integer) the handle's work is enqueued on; wrap it with torch.cuda.ExternalStream to order
        collectives after the render."""
        p = C.c_void_p()
        _check(load_library().amber_hip_pt_stream(self._h, C.byref(p)))
        return p.value or 0

    def device_framebuffer(self):
        p, n = C.c_void_p(), C.c_uint64()
        _check(load_library().amber_hip_pt_device_framebuffer(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def kernel_time(self):
        n, ms = C.c_uint32(), C.c_double()
        _check(load_library().amber_hip_pt_kernel_time(self._h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def build_info(self) -> dict:
        """Engine BVH's tree as create built it: where (BUILD_*), fallback_reason (BUILD_REASON_*), n_nodes, n_leaves, depth, tree_ms, create_ms."""
        b = BuildInfo()
        _check(load_library().amber_hip_pt_build_info(self._h, C.byref(b)))
        return {k: getattr(b, k) for k, _ in BuildInfo._fields_ if k != "pad"}

    def update_objects(self, first: int, kinds, material_index, params, mode: int = UPDATE_REFIT) -> dict:
        """amber_hip_pt_update_objects for callers who hold arrays as HostScene.create_arrays takes them: new geometry for the scene objects
        [first, first + len(kinds)) -- `first` is a SCENE index, i.e. a position in HostScene.flatten() (create_arrays puts the aperture blades in
        front of the caller's objects: lens.first_blade_object, lens.n_blades) -- and engine BVH's tree refitted (UPDATE_REFIT) or rebuilt
        (UPDATE_REBUILD) on the device.  Returns AmberUpdateInfo as a dict.  The framebuffer is not cleared.

        The records are made the way the scene would flatten them: the host object model builds the primitives (triangle normals, unit disk /
        cylinder axes) and flattens them.  Flattening renumbers materials in order of first appearance, so `material_index` cannot be passed
        through; an update keeps every object's material anyway, so the resident (flattened) index is kept and `material_index` only has to be
        consistent with it: objects that had one index still have one index, and different indices stay different.  This builds a temporary
        host scene of the range; callers who already hold flattened records (HostScene.flatten()) use update_flat."""
        kinds, material_index = np.ascontiguousarray(kinds, np.uint32), np.ascontiguousarray(material_index, np.uint32)
        n = len(kinds)
        if n == 0:
            return self.update_flat(first, np.zeros(0, _RECORD), mode)
        if self._resident is None:
            objs, _, _ = self._scene.flatten()
            self._resident = np.frombuffer(objs, dtype=_RECORD)[["kind", "material"]].copy()
        if first < 0 or first + n > len(self._resident):
            raise AmberError(f"update_objects: objects [{first}, {first + n}) are not all in the scene ({len(self._resident)} objects)")
        resident = self._resident[first:first + n]
        if not np.array_equal(resident["kind"], kinds):
            raise AmberError(f"update_objects: object {first + int(np.argmax(resident['kind'] != kinds))}: the kind differs from the resident record's (an update moves geometry only)")
        pairs = np.unique(np.stack([material_index, resident["material"]], 1), axis=0)
        if len(np.unique(pairs[:, 0])) != len(pairs) or len(np.unique(pairs[:, 1])) != len(pairs):
            raise AmberError("update_objects: material_index is not the resident objects' material assignment (an update moves geometry only)")
        # geometry through the host object model: a pinhole scene of the range with one material; its aperture object is dropped again
        tmp = HostScene.create_arrays(kinds, np.zeros(n, np.uint32), params, [(MAT_LAMBERTIAN, (0.5, 0.5, 0.5), 0.0)],
                                      [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1], 0.05, 1.0, 0.01, 0)
        objs, _, lens = tmp.flatten()
        flat = np.frombuffer(objs, dtype=_RECORD)
        keep = np.ones(len(flat), bool)
        keep[lens.first_blade_object:lens.first_blade_object + lens.n_blades] = False
        records = flat[keep].copy()
        tmp.close()
        assert len(records) == n and np.array_equal(records["kind"], kinds)
        records["material"] = resident["material"]
        return self.update_flat(first, records, mode)

    def update_flat(self, first: int, records, mode: int = UPDATE_REFIT, count=None) -> dict:
        """update_objects with the records as one array of AmberFlatObject (64 bytes each: HostScene.flatten()'s layout).  records=None passes a
        null pointer with `count` objects."""
        info = UpdateInfo()
        ptr, n = None, count or 0
        if records is not None:
            records = np.ascontiguousarray(records)
            assert records.itemsize == C.sizeof(FlatObject)
            ptr, n = records.ctypes.data, len(records) if count is None else count
        _check(load_library().amber_hip_pt_update_objects(self._h, first, n, ptr, mode, C.byref(info)))
        return {k: getattr(info, k) for k, _ in UpdateInfo._fields_}

    def update_lens(self, scene_or_lens, mode: int = UPDATE_REFIT) -> dict:
        """amber_hip_pt_update_lens: the camera of a live handle moved.  scene_or_lens is a HostScene -- the same scene with another lens; it is
        flattened and its lens and blade records are taken -- or an explicit (FlatThinLens, records) pair, records being the lens's n_blades
        AmberFlatObject records (HostScene.flatten()'s layout; None passes a null pointer, as a None lens does).  Engine BVH's tree is refitted
        (UPDATE_REFIT) or rebuilt (UPDATE_REBUILD) on the device.  Returns AmberUpdateInfo as a dict, like update_objects.  The framebuffer is
        not cleared."""
        if isinstance(scene_or_lens, HostScene):
            objs, _, lens = scene_or_lens.flatten()
            records = np.frombuffer(objs, dtype=_RECORD)[lens.first_blade_object:lens.first_blade_object + lens.n_blades].copy()
        else:
            lens, records = scene_or_lens
        ptr = None
        if records is not None:
            records = np.ascontiguousarray(records)
            assert records.itemsize == C.sizeof(FlatObject)
            if lens is not None and len(records) < lens.n_blades:
                raise AmberError(f"update_lens: {len(records)} blade records for a lens of {lens.n_blades} blades")
            ptr = records.ctypes.data
        info = UpdateInfo()
        _check(load_library().amber_hip_pt_update_lens(self._h, C.byref(lens) if lens is not None else None, ptr, mode, C.byref(info)))
        return {k: getattr(info, k) for k, _ in UpdateInfo._fields_}

    # ---- the caller's own rays ----------------------------------------------------------------
    @staticmethod
    def _is_torch(a) -> bool:
        return type(a).__module__.split(".")[0] == "torch"

    def _pack_rays(self, origins, dirs, t_max):
        """(packed rays, n, torch module or None).  numpy: an array of AmberRay records.  torch: an (n, 8) float32 tensor on the tensors' device."""
        if self._is_torch(origins) or self._is_torch(dirs):
            import torch
            if not (self._is_torch(origins) and self._is_torch(dirs)) or not origins.is_cuda or origins.device != dirs.device:
                raise AmberError("cast_rays / occluded: origins and dirs must both be numpy arrays or both be torch tensors on the handle's device")
            o, d = origins.reshape(-1, 3).to(torch.float32), dirs.reshape(-1, 3).to(torch.float32)
            if len(o) != len(d):
                raise AmberError("cast_rays / occluded: origins and dirs differ in length")
            packed = torch.zeros((len(o), 8), dtype=torch.float32, device=o.device)
            packed[:, 0:3], packed[:, 4:7] = o, d
            if t_max is None:
                packed[:, 3] = float("inf")
            else:
                packed[:, 3] = t_max if not self._is_torch(t_max) else t_max.to(device=o.device, dtype=torch.float32).reshape(-1)
            return packed, len(o), torch
        o, d = _f32(origins).reshape(-1, 3), _f32(dirs).reshape(-1, 3)
        if len(o) != len(d):
            raise AmberError("cast_rays / occluded: origins and dirs differ in length")
        packed = np.zeros(len(o), _RAY)
        packed["origin"], packed["dir"] = o, d
        packed["t_max"] = np.inf if t_max is None else np.asarray(t_max, np.float32)
        return packed, len(o), None

    def cast_rays(self, origins, dirs, t_max=None):
        """amber_hip_pt_cast_rays: the closest hit of every ray (origins, dirs: (n, 3)) through the handle's engine, reported iff t <= t_max
        (t_max: None = INFINITY, a scalar, or (n,)).  Directions are used as given (t is in units of |dir|).  Returns (object, t, pos, normal):
        object (n,) int32 scene index or -1, t (n,) float32 or NaN, pos and normal (n, 3) float32, zero on a miss.

        numpy arrays go through AMBER_RAYS_HOST (staged by the handle; the call returns with the answer) and come back as numpy arrays.
        torch tensors on the handle's device go zero-copy: they are packed into an (n, 8) float32 tensor whose data_ptr() the engine reads,
        and torch tensors come back.  ORDERING: the engine works on the handle's stream, not on torch's current stream.  Wrap the handle's stream
        -- torch.cuda.ExternalStream(pt.stream()) -- and call this under `with torch.cuda.stream(...)` of it, so that the packing, the query and
        the returned tensors are ordered on one stream; without that this method waits for torch's current stream before the query and for the
        handle's stream after it.  A query enqueued before update_objects answers for the old scene, one enqueued after it for the new one."""
        packed, n, torch = self._pack_rays(origins, dirs, t_max)
        lib = load_library()
        if torch is None:
            hits = np.zeros(n, _RAY_HIT)
            _check(lib.amber_hip_pt_cast_rays(self._h, n, packed.ctypes.data, hits.ctypes.data, RAYS_HOST))
            return hits["object"].copy(), hits["t"].copy(), hits["pos"].copy(), hits["normal"].copy()
        out = torch.empty((n, 8), dtype=torch.float32, device=packed.device)
        with self._on_stream(torch, packed.device):
            _check(lib.amber_hip_pt_cast_rays(self._h, n, packed.data_ptr(), out.data_ptr(), 0))
        return out[:, 1].contiguous().view(torch.int32), out[:, 0].contiguous(), out[:, 2:5].contiguous(), out[:, 5:8].contiguous()

    def occluded(self, origins, dirs, t_max=None):
        """amber_hip_pt_occluded: (n,) bool (numpy) or torch.bool, True iff cast_rays on the same ray would report a hit -- something lies on the
        ray at some t <= t_max.  Engine BVH answers with an any-hit walk that stops at the first such object.  Arguments, memory and ordering as
        cast_rays (torch tensors: wrap PathTracer.stream() in torch.cuda.ExternalStream)."""
        packed, n, torch = self._pack_rays(origins, dirs, t_max)
        lib = load_library()
        if torch is None:
            occ = np.zeros(n, np.uint8)
            _check(lib.amber_hip_pt_occluded(self._h, n, packed.ctypes.data, occ.ctypes.data, RAYS_HOST))
            return occ.astype(bool)
        out = torch.empty(n, dtype=torch.uint8, device=packed.device)
        with self._on_stream(torch, packed.device):
            _check(lib.amber_hip_pt_occluded(self._h, n, packed.data_ptr(), out.data_ptr(), 0))
        return out.to(torch.bool)

    def trace_paths(self, origins, dirs, weights=None, states=None, n_samples: int = 1, max_depth: int = 0):
        """amber_hip_pt_trace_paths: the radiance that comes back along every ray (origins, dirs: (n, 3)) -- n_samples paths per ray through the
        render kernels' bounce loop, each started at (origin, dir, weight) with the ray's sampler stream as the previous sample left it, their
        measurements summed in order.  weights: (n, 3), None = 1.  states: (n,) uint64 sampler states (torch: int64 holding the same bits), None =
        sampler_state(the handle's seed, i, 0); a state of 0 is replaced by 0x9E3779B97F4A7C15.  max_depth: 0 = the handle's, else it replaces
        the handle's for this call.  Returns (rgb, casts, states_after): rgb (n, 3) float32 SUMS over the samples (divide by n_samples for the
        estimate), casts (n,) uint32 (torch: int32, the same bits), states_after (n,) uint64 (torch: int64) to continue the streams with.

        Memory and ordering as cast_rays: numpy arrays go through AMBER_RAYS_HOST and come back as numpy arrays; torch tensors on the handle's
        device go zero-copy (packed into an (n, 16) float32 tensor) and torch tensors come back, ordered on the handle's stream -- call it under
        `with torch.cuda.stream(torch.cuda.ExternalStream(pt.stream()))` to avoid the two waits."""
        lib = load_library()
        if self._is_torch(origins) or self._is_torch(dirs):
            import torch
            if not (self._is_torch(origins) and self._is_torch(dirs)) or not origins.is_cuda or origins.device != dirs.device:
                raise AmberError("trace_paths: origins and dirs must both be numpy arrays or both be torch tensors on the handle's device")
            o, d = origins.reshape(-1, 3).to(torch.float32), dirs.reshape(-1, 3).to(torch.float32)
            n = len(o)
            if len(d) != n:
                raise AmberError("trace_paths: origins and dirs differ in length")
            packed = torch.zeros((n, 16), dtype=torch.float32, device=o.device)
            packed[:, 0:3], packed[:, 4:7] = o, d
            if weights is None:
                packed[:, 8:11] = 1.0
            else:
                packed[:, 8:11] = torch.as_tensor(weights, device=o.device).to(torch.float32).reshape(-1, 3)
            if states is None:
                states = sampler_states(self.seed, np.arange(n), np.zeros(n))
            if not self._is_torch(states):
                states = torch.from_numpy(np.ascontiguousarray(states, np.uint64).view(np.int64))
            packed.view(torch.int64)[:, 6] = states.to(device=o.device, dtype=torch.int64).reshape(-1)
            out = torch.empty((n, 8), dtype=torch.float32, device=o.device)
            with self._on_stream(torch, o.device):
                _check(lib.amber_hip_pt_trace_paths(self._h, n, packed.data_ptr(), out.data_ptr(), n_samples, max_depth, 0))
            return out[:, 0:3].contiguous(), out[:, 3].contiguous().view(torch.int32), out.view(torch.int64)[:, 2].contiguous()
        o, d = _f32(origins).reshape(-1, 3), _f32(dirs).reshape(-1, 3)
        n = len(o)
        if len(d) != n:
            raise AmberError("trace_paths: origins and dirs differ in length")
        packed = np.zeros(n, _PATH_RAY)
        packed["origin"], packed["dir"] = o, d
        packed["weight"] = 1.0 if weights is None else _f32(weights).reshape(-1, 3)
        packed["rng_state"] = sampler_states(self.seed, np.arange(n), np.zeros(n)) if states is None else np.asarray(states, np.uint64).reshape(-1)
        res = np.zeros(n, _PATH_RESULT)
        _check(lib.amber_hip_pt_trace_paths(self._h, n, packed.ctypes.data, res.ctypes.data, n_samples, max_depth, RAYS_HOST))
        return res["rgb"].copy(), res["casts"].copy(), res["rng_state"].copy()

    @contextlib.contextmanager
    def _on_stream(self, torch, device):
        """Around a call that works on torch memory: nothing when torch's current stream IS the handle's stream (everything is ordered already);
        otherwise torch's stream is waited for before the call and the handle's stream after it, also when the call raises."""
        same = torch.cuda.current_stream(device).cuda_stream == self.stream()
        if not same:
            torch.cuda.current_stream(device).synchronize()
        try:
            yield
        finally:
            if not same:
                self.sync()

    @staticmethod
    def _rows_tensor(t, row_bytes: int, what: str) -> None:
        """`what` is raised unless t is a contiguous two-dimensional CUDA tensor with rows of row_bytes bytes"""
        if not PathTracer._is_torch(t) or not t.is_cuda or not t.is_contiguous() or t.dim() != 2 or t.shape[1] * t.element_size() != row_bytes:
            raise AmberError(what)

    def resolve(self, n_samples: int, format: int = RESOLVE_RGB8, mirror: bool = False, out=None):
        """amber_hip_pt_resolve: the band's sums divided by n_samples (RESOLVE_MEAN_F32: float32, 3 channels) or taken through Filmic + Gamma 2.2 to
        8 bits (RESOLVE_RGB8: uint8, 3 channels; RESOLVE_RGBA8: uint8, 4 channels, alpha 255) on the device; the bytes equal tonemap(sum / n).
        mirror: columns written right to left, as the PNG / EXR writers do.

        out=None: returns a numpy array of shape band_shape[:2] + (3 or 4,), through AMBER_RESOLVE_HOST (staged by the handle; the call returns
        with the answer).  out = a contiguous torch tensor on the handle's device, of that dtype and exactly that many elements: zero-copy and
        asynchronous on the handle's stream, `out` is returned.  ORDERING as cast_rays: under `with torch.cuda.stream(ExternalStream(pt.stream()))`
        nothing is waited for; otherwise torch's current stream is waited for before the call and the handle's stream after it."""
        return self._filter("resolve", load_library().amber_hip_pt_resolve, n_samples, None, format, mirror, out)

    def _band_download(self, entry, channels: int) -> np.ndarray:
        """what aov_download(), moments_download() and history_download() share: `channels` float32 per band pixel, rows as download() lays them out"""
        rows, width, _ = self.band_shape
        out = np.zeros((rows, width, channels), np.float32)
        _check(entry(self._h, out.ctypes.data))
        return out

    def _band_pointer(self, entry):
        """what device_aov(), device_moments() and device_history() share: (device pointer, number of band pixels)"""
        p, n = C.c_void_p(), C.c_uint64()
        _check(entry(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    # ---- first-hit AOVs -----------------------------------------------------------------------
    def aov_pass(self, first_sample: int, n_samples: int) -> None:
        """amber_hip_pt_aov_pass: for every pixel of the band and the samples [first_sample, first_sample + n_samples) in this order, the first hit of
        the eye ray the render kernels generate for that pixel and sample adds the hit material's rho, the distance t, the reference's Intersect()
        normal and 1 to the pixel's eight sums (one binary32 addition each; a miss adds nothing).  Asynchronous and stream-ordered on the handle's
        stream like render_pass: a pass enqueued before update_objects / update_lens sees the old scene and lens, one enqueued after it the new
        ones.  Never touches the framebuffer, the ray counter or kernel_time().  The buffer is allocated and zeroed by the first aov_* call."""
        _check(load_library().amber_hip_pt_aov_pass(self._h, first_sample, n_samples))

    def aov_clear(self) -> None:
        """amber_hip_pt_aov_clear: zeroes the AOV buffer (asynchronous, on the handle's stream).  The framebuffer is not cleared; clear() in turn
        leaves the AOV buffer alone."""
        _check(load_library().amber_hip_pt_aov_clear(self._h))

    def aov_download(self) -> np.ndarray:
        """amber_hip_pt_aov_download: a float32 array of shape band_shape[:2] + (8,) in AmberAovPixel's order -- albedo r g b, depth, normal x y z,
        coverage -- rows as download() lays them out.  Raw SUMS: divide by the sample count, or by coverage for a mean over the samples that hit.
        Synchronises."""
        return self._band_download(load_library().amber_hip_pt_aov_download, 8)

    def device_aov(self):
        """amber_hip_pt_device_aov: (device pointer, number of band pixels) of the AOV buffer, 8 float32 per pixel, for zero-copy consumers
        (torch.from_dlpack / a __cuda_array_interface__ wrapper, a denoiser).  ORDERING: the engine works on the handle's stream, not on torch's
        current stream.  Wrap the handle's stream -- torch.cuda.ExternalStream(pt.stream()) -- and read the buffer under `with torch.cuda.stream(...)`
        of it, so that aov_pass and the reader are ordered on one stream; otherwise call sync() first."""
        return self._band_pointer(load_library().amber_hip_pt_device_aov)

    def denoise(self, n_samples: int, levels: int = 5, k_normal: float = 4.0, k_albedo: float = 100.0, k_depth: float = 10.0, k_color: float = 0.25,
                format: int = RESOLVE_RGB8, mirror: bool = False, out=None):
        """amber_hip_pt_denoise: the band's mean image (sums / n_samples) through `levels` levels of the edge-avoiding a-trous filter, guided by the
        AOV buffer (aov_pass the same samples first; a buffer never filled gives all-zero guides and only the colour stop acts), then through
        resolve's output stage: RESOLVE_MEAN_F32 is the filtered image itself, RESOLVE_RGB8 / RESOLVE_RGBA8 its Filmic + Gamma bytes.  The filter is a
        fixed sequence of binary32 operations (include/amber_hip.h states it; tests/denoise_reference.py restates it in numpy).  A tap's weight falls
        to zero where the squared distance of the normals reaches 1 / k_normal, of the albedos 1 / k_albedo, of the colours 1 / k_color (a quarter of
        that at every further level), and where the depths differ by 1 / k_depth of the pixel's depth.  The defaults -- normals about 30 degrees apart,
        albedo 0.1 apart, depth 10 % apart, colour 2.0 apart at level 0 -- are starting points: nobody has measured their quality on this renderer's
        frames.  A band filters within itself (no halo across ranks); a striped handle is refused.  Leaves the framebuffer, the AOV buffer, the ray
        counter and kernel_time() alone.

        out, torch handling and ORDERING exactly as resolve()."""
        params = DenoiseParams(levels=levels, k_normal=k_normal, k_albedo=k_albedo, k_depth=k_depth, k_color=k_color)
        return self._filter("denoise", load_library().amber_hip_pt_denoise, n_samples, params, format, mirror, out)

    def _filter(self, what: str, entry, n_samples: int, params, format: int, mirror: bool, out):
        """the output handling resolve() (params is None: its entry point takes none), denoise(), denoise_variance() and temporal() share"""
        if format not in (RESOLVE_MEAN_F32, RESOLVE_RGB8, RESOLVE_RGBA8):
            raise AmberError(f"{what}: unknown format {format}")
        rows, width, _ = self.band_shape
        channels, flags = (4 if format == RESOLVE_RGBA8 else 3), (RESOLVE_MIRROR_X if mirror else 0)
        head = (self._h, n_samples) if params is None else (self._h, n_samples, C.byref(params))
        if out is None:
            res = np.empty((rows, width, channels), np.float32 if format == RESOLVE_MEAN_F32 else np.uint8)
            _check(entry(*head, format, res.ctypes.data, res.nbytes, flags | RESOLVE_HOST))
            return res
        if not self._is_torch(out):
            raise AmberError(f"{what}: out must be None or a torch tensor on the handle's device")
        import torch
        dtype = torch.float32 if format == RESOLVE_MEAN_F32 else torch.uint8
        if not out.is_cuda or out.dtype != dtype or not out.is_contiguous() or out.numel() != rows * width * channels:
            raise AmberError(f"{what}: out must be a contiguous {dtype} tensor of {rows} x {width} x {channels} elements on the handle's device")
        with self._on_stream(torch, out.device):
            _check(entry(*head, format, out.data_ptr(), out.numel() * out.element_size(), flags))
        return out

    # ---- batch moments and the variance-guided filter ------------------------------------------
    def render_batch(self, first_sample: int, n_samples: int) -> None:
        """amber_hip_pt_render_batch: render_pass(first_sample, n_samples) whose sums B land in a zeroed buffer of their own, then fb = fb + B and the
        luminance Y of B / n_samples into the pixel's moments: m1 += Y, m2 += Y * Y, batches += 1.  Up to one accumulation chunk of samples the
        framebuffer gets render_pass's very bits; a longer batch is summed first and added once.  Rays and kernel_time() count as for render_pass.
        The caller chooses the granularity: four calls of one sample give per-sample moments of a 4-spp frame.  Asynchronous and stream-ordered,
        except that a pass whose record buffer was sized from an estimate is waited for.  n_samples == 0 changes nothing."""
        _check(load_library().amber_hip_pt_render_batch(self._h, first_sample, n_samples))

    def moments_clear(self) -> None:
        """amber_hip_pt_moments_clear: zeroes the moments buffer (asynchronous, on the handle's stream).  The framebuffer is not cleared; clear() in
        turn leaves the moments alone."""
        _check(load_library().amber_hip_pt_moments_clear(self._h))

    def moments_download(self) -> np.ndarray:
        """amber_hip_pt_moments_download: a float32 array of shape band_shape[:2] + (4,) in AmberMomentsPixel's order -- m1, m2, batches, pad -- rows
        as download() lays them out.  Synchronises."""
        return self._band_download(load_library().amber_hip_pt_moments_download, 4)

    def device_moments(self):
        """amber_hip_pt_device_moments: (device pointer, number of band pixels) of the moments buffer, 4 float32 per pixel.  ORDERING as device_aov."""
        return self._band_pointer(load_library().amber_hip_pt_device_moments)

    def denoise_variance(self, n_samples: int, levels: int = 5, k_normal: float = 4.0, k_albedo: float = 100.0, k_depth: float = 10.0, k_lum: float = 16.0,
                         var_radius: int = 3, format: int = RESOLVE_RGB8, mirror: bool = False, out=None):
        """amber_hip_pt_denoise_variance: denoise() with the colour stop replaced by a luminance stop that the variance of the mean scales.  That variance
        comes from the moments render_batch keeps (render the frame as batches: four render_batch(s, 1) for a 4-spp frame), pooled over the
        (2 * var_radius + 1)^2 neighbours the guide stops let through, blurred 3 x 3 and filtered along with the colour.  A tap's weight falls to zero
        where the luminances differ by sqrt(k_lum) standard deviations of the estimate -- four with k_lum = 16; the guide stops are denoise()'s.  A
        fixed sequence of binary32 operations (include/amber_hip.h states it; tests/denoise_variance_reference.py restates it in numpy).  The defaults
        are starting points: nobody has tuned them on this renderer's frames (EXPERIMENTS.md has what was measured).  A band filters within itself; a
        striped handle is refused.  Leaves the framebuffer, the AOV buffer, the moments, the ray counter and kernel_time() alone.

        out, torch handling and ORDERING exactly as resolve()."""
        params = DenoiseVarianceParams(levels=levels, k_normal=k_normal, k_albedo=k_albedo, k_depth=k_depth, k_lum=k_lum, var_radius=var_radius)
        return self._filter("denoise_variance", load_library().amber_hip_pt_denoise_variance, n_samples, params, format, mirror, out)

    # ---- reprojected frame history ---------------------------------------------------------------
    def temporal(self, n_samples: int, levels: int = 5, max_history: int = 32, k_normal: float = 4.0, k_albedo: float = 100.0, k_depth: float = 10.0,
                 k_color: float = 0.25, format: int = RESOLVE_RGB8, mirror: bool = False, out=None):
        """amber_hip_pt_temporal: this frame's mean (sums / n_samples) accumulated into the handle's per-pixel history, then `levels` levels of
        denoise()'s filter on the accumulated colour (0: none), then resolve's output stage.  The frame loop: update_lens / update_objects, clear(),
        render_pass or lt_render_pass of this frame's samples (a fresh first_sample per frame), aov_clear(), aov_pass, temporal(n_samples).  The
        previous history is reprojected through the previous lens (bilinear, four taps; an unchanged lens reprojects every pixel to itself, so a
        static camera is an exact running mean) and a tap is accepted only where the previous guide passes denoise()'s normal, albedo and depth
        stops; a pixel without an accepted tap starts again.  The history length is capped at max_history, from where the blend is exponential.  A
        fixed sequence of binary32 operations (include/amber_hip.h states it; tests/temporal_reference.py restates it in numpy).  The filtered colour
        is not fed back.  The defaults are starting points nobody has tuned (EXPERIMENTS.md has what was measured).  A band reprojects and filters
        within itself; a striped handle is refused.  Leaves the framebuffer, the AOV buffer, the moments, the ray counter and kernel_time() alone.

        out, torch handling and ORDERING exactly as resolve()."""
        params = TemporalParams(levels=levels, max_history=max_history, k_normal=k_normal, k_albedo=k_albedo, k_depth=k_depth, k_color=k_color)
        return self._filter("temporal", load_library().amber_hip_pt_temporal, n_samples, params, format, mirror, out)

    def temporal_reset(self) -> None:
        """amber_hip_pt_temporal_reset: empties the history (asynchronous, on the handle's stream): the next temporal() is a first call.  clear(),
        aov_clear(), update_objects() and update_lens() leave the history alone."""
        _check(load_library().amber_hip_pt_temporal_reset(self._h))

    def history_download(self) -> np.ndarray:
        """amber_hip_pt_history_download: a float32 array of shape band_shape[:2] + (8,) in AmberHistoryPixel's order -- colour r g b, length, m1, m2,
        two pads -- rows as download() lays them out.  A history never used, or emptied, reads as zeros.  Synchronises."""
        return self._band_download(load_library().amber_hip_pt_history_download, 8)

    def device_history(self):
        """amber_hip_pt_device_history: (device pointer, number of band pixels) of the CURRENT history buffer, 8 float32 per pixel; the next temporal()
        makes the other buffer current, so ask again after every call.  ORDERING as device_aov."""
        return self._band_pointer(load_library().amber_hip_pt_device_history)

    def lt_trace(self, first_sample: int, n_samples: int, capacity: int = 1 << 16, paths=None):
        """Light tracing (algorithm_lt.cc): splats of W*H light paths per pass (or of the light paths [paths[0], paths[1])),
        sorted (pass, path, bounce).  Returns (structured numpy array of records, ray count)."""
        dt = SPLAT_DTYPE
        while True:
            out = np.zeros(capacity, dt)
            n, rays = C.c_uint32(), C.c_uint64()
            if paths is None:
                rc = load_library().amber_hip_lt_trace(self._h, first_sample, n_samples, out.ctypes.data, capacity, C.byref(n), C.byref(rays))
            else:
                rc = load_library().amber_hip_lt_trace_range(self._h, first_sample, n_samples, paths[0], paths[1], out.ctypes.data, capacity,
                                                             C.byref(n), C.byref(rays))
            if rc == -4 and n.value > capacity:
                capacity = n.value
                continue
            _check(rc)
            return out[: n.value], rays.value

    def lt_render_pass(self, first_sample: int, n_samples: int) -> dict:
        """amber_hip_lt_render_pass: the light-tracing passes [first_sample, first_sample + n_samples) into the handle's framebuffer on the device, in the
        reference's order -- per pass a pass image summed from +0 in (path, bounce) order, pass images added to the framebuffer in pass order, bit for
        bit what adding lt_trace's records on the host gives (include/amber_hip.h states it; tests/lt_accumulate_reference.py restates it in numpy).
        The framebuffer is render_pass's and is not cleared; download / resolve / denoise / device_framebuffer work on it as they are, and
        resolve(n) after n passes is the mean `algorithm="lt"` returns.  Any split of the passes over calls leaves the same bits.  The ray counter
        grows by lt_trace's ray count and kernel_time() counts the trace launches.  Waits for the stream.  Whole-frame handles only.  Returns
        AmberLtPassInfo as a dict: n_splats, n_rays, n_launches, n_repeats (launches repeated after the handle's splat buffer,
        LT_SPLAT_CAPACITY0 records at first, had to grow), longest_run (most records of one pixel in one pass)."""
        info = LtPassInfo()
        _check(load_library().amber_hip_lt_render_pass(self._h, first_sample, n_samples, C.byref(info)))
        return {k: int(getattr(info, k)) for k, _ in LtPassInfo._fields_ if k != "pad"}

    def lt_trace_photons(self, first_sample: int, n_samples: int, surfaces: int = PHOTON_DIFFUSE, paths=None, out=None):
        """amber_hip_lt_trace_photons: the vertices of the light paths lt_trace traces -- passes [first_sample, first_sample + n_samples) of the light paths
        [paths[0], paths[1]) (None: all W*H) -- on the surfaces `surfaces` selects (PHOTON_* bits), as AmberPhoton records (PHOTON_DTYPE) in ascending
        (sample, path, bounce) order: pos, normal and object of the hit, dir_out = -ray direction, weight = the path weight on arrival (divide by the
        number of paths for PhotonMap::Build's photons), bounce counted from 1.  include/amber_hip.h states it; tests/photon_reference.py restates it.
        Returns (records, info): info is AmberPhotonInfo as a dict (n_photons, n_written, n_rays, n_launches, n_repeats).
        out=None: a counting call, then a filling call into a numpy structured array of exactly that size, which is returned.
        out = a numpy array of PHOTON_DTYPE: filled through AMBER_PHOTONS_HOST; its first n_written records are returned (a view).
        out = a torch tensor on the handle's device (contiguous, rows of 64 bytes, e.g. (capacity, 16) float32), or (device pointer, capacity): written
        zero-copy on the handle's stream (ORDERING as cast_rays; the call waits for the handle's stream before it returns); the tensor's first n_written
        rows, or n_written, are returned.  A buffer that is too small raises AmberError with .code == -4 and .info["n_photons"] = the records needed."""
        lib = load_library()
        begin, end = (0, self.sensor.width * self.sensor.height) if paths is None else (int(paths[0]), int(paths[1]))
        info = PhotonInfo()

        def call(ptr, capacity, flags):
            rc = lib.amber_hip_lt_trace_photons(self._h, first_sample, n_samples, begin, end, surfaces, ptr, capacity, C.byref(info), flags)
            d = {k: int(getattr(info, k)) for k, _ in PhotonInfo._fields_}
            if rc != 0:
                try:
                    _check(rc)
                except AmberError as e:
                    e.code, e.info = rc, d
                    raise
            return d

        if out is None:
            need = call(None, 0, PHOTONS_HOST)["n_photons"]
            out = np.zeros(need, PHOTON_DTYPE)
            d = call(out.ctypes.data if need else None, need, PHOTONS_HOST)
            return out, d
        if isinstance(out, np.ndarray):
            if out.dtype != PHOTON_DTYPE or not out.flags.c_contiguous or out.ndim != 1:
                raise AmberError("lt_trace_photons: out must be a contiguous one-dimensional numpy array of PHOTON_DTYPE")
            d = call(out.ctypes.data if len(out) else None, len(out), PHOTONS_HOST)
            return out[: d["n_written"]], d
        if self._is_torch(out):
            import torch
            self._rows_tensor(out, 64, "lt_trace_photons: out must be a contiguous torch tensor on the handle's device with rows of 64 bytes")
            with self._on_stream(torch, out.device):
                d = call(out.data_ptr() if out.shape[0] else None, out.shape[0], 0)
            return out[: d["n_written"]], d
        ptr, capacity = out
        d = call(ptr, capacity, 0)
        return d["n_written"], d

    def pm_build(self, photons, cell_size: float) -> dict:
        """amber_hip_pm_build: the handle's photon map -- a uniform grid of cells of `cell_size` (doubled until the grid fits 1024 cells per axis and
        2^22 in all) over `photons`, replacing the map before.  Only pos, dir_out and weight of the records are read; photons with a non-finite position
        are dropped.  include/amber_hip.h states it; tests/photon_map_reference.py restates it.  Returns AmberPhotonMapInfo as a dict.
        photons = a numpy array of PHOTON_DTYPE (what lt_trace_photons returns): through AMBER_PHOTONS_HOST.
        photons = a torch tensor on the handle's device (contiguous, rows of 64 bytes), or (device pointer, count): read zero-copy on the handle's stream
        (ORDERING as cast_rays).  Either way the buffer is free when the call returns: the map keeps its own copy, and the call waits for the stream."""
        lib = load_library()
        info = PhotonMapInfo()

        def call(ptr, n, flags):
            _check(lib.amber_hip_pm_build(self._h, ptr, n, cell_size, flags, C.byref(info)))
            d = {k: getattr(info, k) for k, _ in PhotonMapInfo._fields_}
            d["dims"], d["lo"], d["hi"] = tuple(info.dims), tuple(info.lo), tuple(info.hi)
            return d

        if isinstance(photons, np.ndarray):
            rec = np.ascontiguousarray(photons, PHOTON_DTYPE).reshape(-1)
            return call(rec.ctypes.data if len(rec) else None, len(rec), PHOTONS_HOST)
        if self._is_torch(photons):
            import torch
            self._rows_tensor(photons, 64, "pm_build: photons must be a contiguous torch tensor on the handle's device with rows of 64 bytes")
            with self._on_stream(torch, photons.device):
                return call(photons.data_ptr() if photons.shape[0] else None, photons.shape[0], 0)
        ptr, n = photons
        return call(ptr, n, 0)

    def pm_gather(self, queries, k: int = 0, raw: bool = False, out=None):
        """amber_hip_pm_gather: for every query (GATHER_QUERY_DTYPE: pos, radius | normal, object | dir_out | weight) the photons of the handle's map within
        `radius` -- the k nearest of them when k > 0 and there are more -- and rgb = (sum(photon.weight * rho * fs) * kern) * weight, kern = 1 / (pi radius^2)
        (raw=True: the plain sum).  Returns GATHER_RESULT_DTYPE records: rgb, n_used, r2_used, n_in_radius.
        queries = a numpy array of GATHER_QUERY_DTYPE: through AMBER_RAYS_HOST; `out` (optional) a numpy array of GATHER_RESULT_DTYPE of the same length.
        queries = a torch tensor on the handle's device (contiguous, rows of 64 bytes, e.g. (n, 16) float32): zero-copy on the handle's stream (ORDERING as
        cast_rays); `out` (optional) a tensor with rows of 32 bytes; an (n, 8) float32 tensor comes back."""
        lib = load_library()
        flags = PM_RAW_SUM if raw else 0
        if self._is_torch(queries):
            import torch
            self._rows_tensor(queries, 64, "pm_gather: queries must be a contiguous torch tensor on the handle's device with rows of 64 bytes")
            n = queries.shape[0]
            if out is None:
                out = torch.empty((n, 8), dtype=torch.float32, device=queries.device)
            else:
                self._rows_tensor(out if self._is_torch(out) and out.shape[:1] == (n,) else None, 32,
                                  "pm_gather: out must be a contiguous torch tensor on the handle's device with a row of 32 bytes per query")
            with self._on_stream(torch, queries.device):
                _check(lib.amber_hip_pm_gather(self._h, n, queries.data_ptr() if n else None, out.data_ptr() if n else None, k, flags))
            return out
        q = np.ascontiguousarray(queries, GATHER_QUERY_DTYPE).reshape(-1)
        if out is None:
            out = np.zeros(len(q), GATHER_RESULT_DTYPE)
        elif not isinstance(out, np.ndarray) or out.dtype != GATHER_RESULT_DTYPE or not out.flags.c_contiguous or out.shape != (len(q),):
            raise AmberError("pm_gather: out must be a contiguous numpy array of GATHER_RESULT_DTYPE with a record per query")
        _check(lib.amber_hip_pm_gather(self._h, len(q), q.ctypes.data if len(q) else None, out.ctypes.data if len(q) else None, k, RAYS_HOST | flags))
        return out

    def pm_release(self) -> None:
        """amber_hip_pm_release: waits for the handle's stream and frees the photon map and its scratch; pm_gather is an error until the next pm_build."""
        _check(load_library().amber_hip_pm_release(self._h))

    # ---- known-answer entry points -----------------------------------------------------------
    def kat_pm_stage_ms(self):
        """Lab build: (build ms, gather ms) of pm_build / pm_gather by hipEvents since the previous call; the first call switches the timing on."""
        a, b = C.c_double(), C.c_double()
        _check(load_library().amber_hip_kat_pm_stage_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def kat_bsdf(self, objects, normals, dirs_out, dirs_in):
        """Lab build: rho * SymmetricBSDF(normal, dir_out, dir_in) of the material of objects[i] (scene object indices), (n, 3) float32."""
        o = np.ascontiguousarray(objects, np.int32)
        nn, dd, di = _f32(normals).reshape(-1, 3), _f32(dirs_out).reshape(-1, 3), _f32(dirs_in).reshape(-1, 3)
        out = np.empty((len(o), 3), np.float32)
        _check(load_library().amber_hip_kat_bsdf(self._h, len(o), o.ctypes.data, nn.ctypes.data, dd.ctypes.data, di.ctypes.data, out.ctypes.data))
        return out

    def kat_photon_stage_ms(self):
        """Lab build: (trace ms, sort ms, gather ms) of lt_trace_photons by hipEvents since the previous call; the first call switches the timing on."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        _check(load_library().amber_hip_kat_photon_stage_ms(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def kat_lt_accumulate(self, records) -> None:
        """Lab build: lt_render_pass's device path (order by (pixel, pass, path, bounce), ordered sum) on the caller's records -- a structured array of
        lt_trace's dtype, in any order -- into the framebuffer."""
        rec = np.ascontiguousarray(records, SPLAT_DTYPE)
        _check(load_library().amber_hip_kat_lt_accumulate(self._h, rec.ctypes.data if len(rec) else None, len(rec)))

    def kat_accumulate(self, n_samples: int, q, rgb, n_waves: int = 4, rec_capacity: int = 0, rays: int = 0) -> dict:
        """Lab build: one path launch over n_samples samples of the band whose records are the caller's -- q[i] = band pixel * n_samples + sample,
        0xffffffff for a lane that emits nothing, rgb[i] its measurement -- through the product's emitters, reduction and repeat into the framebuffer
        (include/amber_hip_lab.h; tests/path_accumulate_reference.py restates the sum).  Returns AmberAccumulateInfo as a dict."""
        qq = np.ascontiguousarray(q, np.uint32).reshape(-1)
        cc = _f32(rgb).reshape(-1, 3)
        assert len(qq) == len(cc)
        info = AccumulateInfo()
        _check(load_library().amber_hip_kat_accumulate(self._h, n_samples, qq.ctypes.data if len(qq) else None, cc.ctypes.data if len(qq) else None,
                                                       len(qq), n_waves, rec_capacity, rays, C.byref(info)))
        return {k: int(getattr(info, k)) for k, _ in AccumulateInfo._fields_}

    def kat_scout_flags(self, first_sample: int, n_samples: int):
        """Lab build: (flagged, scouts) -- a bool per path q = band pixel * n_samples + sample offset of one launch: the scout flagged it (it ends on a
        light, or it is suspect), taken after the scout and before the replay; scouts False: the handle renders with the full kernel, nothing is flagged."""
        n_paths = len(self.row_index) * self.sensor.width * n_samples
        words = np.zeros((n_paths + 31) // 32 + 1, np.uint32)
        scouts, bound0 = C.c_uint32(), C.c_uint32()
        _check(load_library().amber_hip_kat_scout_flags(self._h, first_sample, n_samples, words.ctypes.data, len(words), C.byref(scouts), C.byref(bound0)))
        self.scout_bound0 = int(bound0.value)           # the host's bound of log2 |eye weight|, sixteenths of a bit (scout_bound.h)
        return np.unpackbits(words.view(np.uint8), bitorder="little")[:n_paths].astype(bool), bool(scouts.value)

    def kat_lt_stage_ms(self):
        """Lab build: (sort ms, sum ms) of lt_render_pass's device path since the previous call; the first call switches the timing on."""
        a, b = C.c_double(), C.c_double()
        _check(load_library().amber_hip_kat_lt_stage_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def kat_cast(self, origins, dirs):
        o, d = _f32(origins).reshape(-1, 3), _f32(dirs).reshape(-1, 3)
        n = len(o)
        obj, t = np.empty(n, np.int32), np.empty(n, np.float32)
        pos, nrm = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        _check(load_library().amber_hip_kat_cast(self._h, n, o.ctypes.data, d.ctypes.data, obj.ctypes.data, t.ctypes.data,
                                                 pos.ctypes.data, nrm.ctypes.data))
        return obj, t, pos, nrm

    def kat_phase_a(self, origins, dirs, axis_loops: bool = True):
        """Lab build: Phase A's candidate masks of the rays, uint32 [n, n_groups] (amber_hip_lab.h); axis_loops False: the general slab loop."""
        o, d = _f32(origins).reshape(-1, 3), _f32(dirs).reshape(-1, 3)
        n = len(o)
        out, groups = np.zeros(4 * n, np.uint32), C.c_uint32()
        _check(load_library().amber_hip_kat_phase_a(self._h, n, o.ctypes.data, d.ctypes.data, int(bool(axis_loops)), out.ctypes.data, out.size, C.byref(groups)))
        return out[:n * groups.value].reshape(n, groups.value)

    def kat_sample(self, material, normals, dirs_out, rng_state, importance: bool = False):
        """SampleLight of material[i], or (importance) SampleImportance, the light-tracing side: bit 31 of the index (amber_hip_lab.h)."""
        m = np.ascontiguousarray(material, np.uint32) | np.uint32(0x80000000 if importance else 0)
        nn, dd = _f32(normals).reshape(-1, 3), _f32(dirs_out).reshape(-1, 3)
        st = np.ascontiguousarray(rng_state, np.uint64).copy()
        n = len(m)
        di, w = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        _check(load_library().amber_hip_kat_sample(self._h, n, m.ctypes.data, nn.ctypes.data, dd.ctypes.data, st.ctypes.data,
                                                   di.ctypes.data, w.ctypes.data))
        return di, w, st

    def kat_eye(self, pixel, sample):
        p, s = np.ascontiguousarray(pixel, np.uint32), np.ascontiguousarray(sample, np.uint32)
        out = np.empty((len(p), 7), np.float32)
        _check(load_library().amber_hip_kat_eye(self._h, len(p), p.ctypes.data, s.ctypes.data, out.ctypes.data))
        return out

    def kat_light_ray(self, rng_state):
        """GenerateLightRay from every XorShift state: (origin, dir, weight, position in the light table, state after)."""
        st = np.ascontiguousarray(rng_state, np.uint64).copy()
        n = len(st)
        o, d, w = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        light = np.empty(n, np.uint32)
        _check(load_library().amber_hip_kat_light_ray(self._h, n, st.ctypes.data, o.ctypes.data, d.ctypes.data, w.ctypes.data, light.ctypes.data))
        return o, d, w, light, st

    def kat_lens_response(self, position, direction_out):
        """LensResponse of every ray: (reached, pixel index, value); pixel and value are 0 where reached is 0."""
        p, d = _f32(position).reshape(-1, 3), _f32(direction_out).reshape(-1, 3)
        n = len(p)
        reached, pixel, value = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.float32)
        _check(load_library().amber_hip_kat_lens_response(self._h, n, p.ctypes.data, d.ctypes.data, reached.ctypes.data, pixel.ctypes.data,
                                                          value.ctypes.data))
        return reached, pixel, value

    def kat_radiance(self, material, normals, dirs_out):
        """Radiance() of material[i] (index into the handle's material table) for every (normal, dir_out)."""
        m = np.ascontiguousarray(material, np.uint32)
        nn, dd = _f32(normals).reshape(-1, 3), _f32(dirs_out).reshape(-1, 3)
        out = np.empty((len(m), 3), np.float32)
        _check(load_library().amber_hip_kat_radiance(self._h, len(m), m.ctypes.data, nn.ctypes.data, dd.ctypes.data, out.ctypes.data))
        return out

    def kat_trace(self, pixel, sample, max_bounces: int = 16):
        p, s = np.ascontiguousarray(pixel, np.uint32), np.ascontiguousarray(sample, np.uint32)
        rec = np.zeros((len(p), max_bounces, 11), np.uint32)
        casts = np.zeros(len(p), np.uint32)
        _check(load_library().amber_hip_kat_trace(self._h, len(p), p.ctypes.data, s.ctypes.data, max_bounces, rec.ctypes.data,
                                                  casts.ctypes.data))
        return rec, casts

    def kat_traversal_rate(self, origins, dirs, waves: int = 5, refill_min: int = 16, repeats: int = 3, rounds=None):
        """Engine BVH's traversal alone: returns (object index, t, best kernel ms) for the rays; `rounds` (uint32 array of len(rays),
        optional) receives the number of wave rounds each ray was in flight for."""
        o, d = _f32(origins).reshape(-1, 3), _f32(dirs).reshape(-1, 3)
        n = len(o)
        obj, t, ms = np.empty(n, np.int32), np.empty(n, np.float32), C.c_double()
        _check(load_library().amber_hip_kat_traversal_rate(self._h, n, o.ctypes.data, d.ctypes.data, waves, refill_min, repeats, t.ctypes.data,
                                                           obj.ctypes.data, C.byref(ms), rounds.ctypes.data if rounds is not None else None))
        return obj, t, ms.value

    def kat_signatures(self, first_sample: int, n_samples: int) -> np.ndarray:
        """(rows, width, n_samples) uint64: low word = hash of the path's hit-object sequence, high word = hash of its hit distances."""
        rows, width, _ = self.band_shape
        out = np.zeros((rows, width, n_samples), np.uint64)
        _check(load_library().amber_hip_kat_signatures(self._h, first_sample, n_samples, out.ctypes.data))
        return out

    def pixel_masks(self):
        """(masks (rows, width) uint32, duration of pixel_mask_kernel in ms): the candidate mask of every band pixel's eye rays (two-phase engine)."""
        rows, width, _ = self.band_shape
        masks = np.zeros((rows, width), np.uint32)
        ms = C.c_double()
        _check(load_library().amber_hip_kat_pixel_masks(self._h, masks.ctypes.data, None, None, C.byref(ms)))
        return masks, ms.value

    def object_slots(self, n_objects: int):
        """(filter-program slot (mask bit) of every scene object, 0xffffffff = none; mask of the slots that are candidates of every ray -- objects
        without a filter record and the aperture blades).  Works with AMBER_PIXEL_MASK=0 and on an empty band: it does not need the mask kernel."""
        slots = np.zeros(n_objects, np.uint32)
        always = C.c_uint32()
        _check(load_library().amber_hip_kat_pixel_masks(self._h, None, slots.ctypes.data, C.byref(always), None))
        return slots, always.value

    def bvh_dump(self) -> dict:
        """Engine BVH's tree as the device holds it (lab build): nodes (n, 8) uint32 -- six plane words (min | max << 16: left x y z, right x y z),
        then the left and right child references (as int32: >= 0 a node, < 0 leaf -(ref + 1) = first * 16 + all_triangles * 8 + all_spheres * 4 + count);
        prims: leaf slot -> object index; root, depth, gmin, step, reach: plane = gmin + binary16 value * step."""
        info = BvhDumpInfo()
        _check(load_library().amber_hip_kat_bvh_dump(self._h, None, 0, None, 0, C.byref(info)))
        nodes, prims = np.zeros((info.n_nodes, 8), np.uint32), np.zeros(info.n_prims, np.uint32)
        _check(load_library().amber_hip_kat_bvh_dump(self._h, nodes.ctypes.data, info.n_nodes, prims.ctypes.data, info.n_prims, C.byref(info)))
        return dict(nodes=nodes, prims=prims, root=int(info.root), depth=int(info.depth), gmin=np.array(info.gmin[:], np.float32),
                    step=np.array(info.step[:], np.float32), reach=np.array(info.reach[:], np.float32))

    def render_signatures(self, first_sample: int, n_samples: int) -> np.ndarray:
        """kat_signatures' layout and meaning, produced by the PRODUCT render kernel (its signature instantiation)."""
        rows, width, _ = self.band_shape
        out = np.zeros((rows, width, n_samples), np.uint64)
        _check(load_library().amber_hip_pt_signatures(self._h, first_sample, n_samples, out.ctypes.data))
        return out

    def close(self):
        if getattr(self, "_h", None):
            load_library().amber_hip_pt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kat_math(mode: int, x, device: int = 0) -> np.ndarray:
    """The engine's sin/cos/pow on device: mode 0 sincos(x[i]) -> (n,2) ; mode 1 pow(x[i,0], x[i,1]) -> (n,) ;
    mode 2 / 3: x[i]^4 / x[i]^5 in binary64 -> (n,) float64."""
    x = _f32(x)
    n = len(x)
    out = np.empty((n,) if mode == 1 else (n, 2), np.float32)
    _check(load_library().amber_hip_kat_math(device, mode, n, x.ctypes.data, out.ctypes.data))
    return out.view(np.float64).reshape(n) if mode >= 2 else out


def kat_division(mode: int, x, device: int = 0) -> np.ndarray:
    """The engine's shared-denominator division on device, x = (n, 4) groups {a, b, c, d} -> (n, 3): mode 0 a/d, b/d, c/d through one
    reciprocal (shared_div.h, with its fallback); mode 1 the plain operators; mode 2 / 3 Normalize({a, b, c}) in the shared / the plain form."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 4)
    n = len(x)
    out = np.empty((n, 3), np.float32)
    _check(load_library().amber_hip_kat_division(device, mode, n, x.ctypes.data, out.ctypes.data))
    return out


class SqrtSweep(C.Structure):
    """AmberSqrtSweep (include/amber_hip_lab.h)."""
    _fields_ = [("mismatches", C.c_uint64), ("in_range", C.c_uint64), ("n_offenders", C.c_uint32), ("offenders", C.c_uint32 * 8),
                ("seed_low", C.c_int32), ("seed_high", C.c_int32)]


def kat_sqrt(mode: int, x, device: int = 0) -> np.ndarray:
    """The engine's square root from one v_rsq_f32 seed on device (exact_sqrt.h): mode 0 the guarded fast form, mode 1 __builtin_sqrtf, x (n,) -> (n,);
    mode 2 / 3 Normalize in the fused / the plain form, x (n, 3) -> (n, 3); mode 4 two roots under one guard, x (n, 2) -> (n, 2)."""
    width = 1 if mode <= 1 else (3 if mode <= 3 else 2)
    x = np.ascontiguousarray(x, np.float32).reshape(-1, width)
    out = np.empty_like(x)
    _check(load_library().amber_hip_kat_sqrt(device, mode, len(x), x.ctypes.data, out.ctypes.data))
    return out.reshape(-1) if width == 1 else out


def kat_sqrt_sweep(first_bits: int, count: int, device: int = 0) -> dict:
    """Mode 0 against mode 1 of kat_sqrt over the bit patterns [first_bits, first_bits + count), generated on the device: the number of
    mismatches, the first offending patterns, the patterns in the fast form's range and v_rsq_f32's extreme distances (ulp) from the nearest float."""
    r = SqrtSweep()
    _check(load_library().amber_hip_kat_sqrt_sweep(device, first_bits, count, C.byref(r)))
    return {"mismatches": int(r.mismatches), "in_range": int(r.in_range), "offenders": [int(b) for b in r.offenders[:min(int(r.n_offenders), 8)]],
            "seed_low": int(r.seed_low), "seed_high": int(r.seed_high)}


MATH_PORTABLE, MATH_GLIBC = 1, 2


def math_mode() -> int:
    """amber_hip_math_mode(): MATH_GLIBC for the product build, MATH_PORTABLE for -DAMBER_BUILD_PORTABLE_MATH measurement builds."""
    return int(load_library().amber_hip_math_mode())


def tonemap(image) -> np.ndarray:
    """Filmic -> Gamma 2.2 -> 8-bit (postprocess/filmic.cc, gamma.cc), image (H, W, 3) float32."""
    img = _f32(image)
    h, w, _ = img.shape
    out = np.empty((h, w, 3), np.uint8)
    _check(load_library().amber_host_tonemap(img.ctypes.data, w, h, out.ctypes.data), host=True)
    return out


def export(image, png_path=None, exr_path=None) -> None:
    """cli::ExportPNG (tone-mapped) / cli::ExportEXR (raw), x-mirrored as the reference writes them."""
    img = _f32(image)
    h, w, _ = img.shape
    _check(load_library().amber_host_export(img.ctypes.data, w, h, png_path.encode() if png_path else None,
                                            exr_path.encode() if exr_path else None), host=True)

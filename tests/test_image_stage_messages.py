"""The refusals of the image stage -- amber_hip_pt_resolve, _denoise, _denoise_variance, _temporal and their nine companion calls -- pinned to the
byte: the return code, the whole amber_hip_last_error() text and, where a call breaks two rules at once, which of them is reported.  The other
suites of the stage assert the code and that the entry point's name is in the message; the host code of the four calls shares its checks
(csrc/hip/image_stage.inc), and this test is what keeps their texts and their order where they are.

The texts are written out here; they were recorded from the library before the checks were shared.  Every message starts with the entry point's
name and a colon, which `refused` puts in front.  Every call here fails before it touches the device, or is a no-op on an empty band: no kernel
runs except what creating the three handles enqueues."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EINVAL = -1
W, H = 20, 6
RESOLVE = "amber_hip_pt_resolve"
# entry point -> (params struct, its fourth constant, its reserved words, the lowest `levels` it takes)
FILTERS = {"amber_hip_pt_denoise": ("DenoiseParams", "k_color", 3, 1),
           "amber_hip_pt_denoise_variance": ("DenoiseVarianceParams", "k_lum", 2, 1),
           "amber_hip_pt_temporal": ("TemporalParams", "k_color", 2, 0)}
STRIPED = "a striped handle's local rows are not neighbours in the frame; filter a contiguous band"
ALIGNED = "a device pointer for MEAN_F32 or RGBA8 must be 4-byte aligned"


def test_every_refusal_keeps_its_code_its_text_and_its_place_in_the_order(amber):
    lib = amber.load_library()
    hs, sensor = amber.HostScene.cornell_box(), amber.Sensor.default(W, H)
    whole = amber.PathTracer(hs, sensor, seed=1)
    striped = amber.PathTracer(hs, sensor, seed=1, rows=(0, H), stripe=(1, 2))            # local rows 0, 2, 4
    empty = amber.PathTracer(hs, sensor, seed=1, rows=(3, 3))
    assert whole.band_shape[:2] == (6, 20) and striped.band_shape[:2] == (3, 20) and empty.band_shape[:2] == (0, 20)
    MEAN, RGB8, RGBA8, HOST, MIRROR = amber.RESOLVE_MEAN_F32, amber.RESOLVE_RGB8, amber.RESOLVE_RGBA8, amber.RESOLVE_HOST, amber.RESOLVE_MIRROR_X
    buf = np.full(W * H * 12 + 16, 0xAB, np.uint8)
    p = buf.ctypes.data
    assert p % 4 == 0

    def params(name, **over):
        struct, k4, n_reserved, _ = FILTERS[name]
        fields = dict(levels=5, k_normal=4.0, k_albedo=100.0, k_depth=10.0)
        fields[k4] = 0.25
        if name == "amber_hip_pt_denoise_variance":
            fields["var_radius"] = 3
        if name == "amber_hip_pt_temporal":
            fields["max_history"] = 32
        reserved = over.pop("reserved", (0,) * n_reserved)
        fields.update(over)
        return ctypes.byref(getattr(amber, struct)(reserved=(ctypes.c_uint32 * n_reserved)(*reserved), **fields))

    def call(name, h, n_samples, prm, fmt, out, n_bytes, flags):
        head = (h, n_samples) if name == RESOLVE else (h, n_samples, prm)
        return getattr(lib, name)(*head, fmt, out, n_bytes, flags)

    def refused(tail, name, h, n_samples, prm, fmt, out, n_bytes, flags):
        assert call(name, h, n_samples, prm, fmt, out, n_bytes, flags) == EINVAL, (name, tail)
        assert lib.amber_hip_last_error() == (name + ": " + tail).encode(), (name, tail)

    for name in [RESOLVE] + list(FILTERS):
        ok = None if name == RESOLVE else params(name)
        # ---- the handle, the sample count
        refused("null handle", name, None, 8, ok, RGB8, p, 360, HOST)
        refused("null handle", name, None, 0, None, 3, None, 0, 4)                        # ... comes first whatever else is wrong
        refused("n_samples is 0", name, whole._h, 0, ok, RGB8, p, 360, HOST)
        refused("n_samples is 0", name, whole._h, 0, ok, 3, None, 1, 4)
        # ---- the output arguments: format, flag bits, (striped,) out_bytes, empty band, null pointer, alignment
        refused("unknown format 3", name, whole._h, 8, ok, 3, p, 360, HOST)
        refused("unknown format 4294967295", name, whole._h, 8, ok, 0xffffffff, p, 360, HOST)
        refused("unknown format 3", name, whole._h, 8, ok, 3, p, 359, HOST)                # bad format and bad out_bytes: the format
        refused("unknown format 3", name, whole._h, 8, ok, 3, p, 360, HOST | 4)
        refused("unknown flag bits", name, whole._h, 8, ok, RGB8, p, 360, HOST | 4)
        refused("unknown flag bits", name, whole._h, 8, ok, RGB8, p, 360, 0x80000000)
        refused("unknown flag bits", name, whole._h, 8, ok, RGB8, None, 359, MIRROR | 8)
        refused("out_bytes is 359, the band takes exactly 360 (6 rows of 20 pixels, 3 bytes each)", name, whole._h, 8, ok, RGB8, p, 359, HOST)
        refused("out_bytes is 1439, the band takes exactly 1440 (6 rows of 20 pixels, 12 bytes each)", name, whole._h, 8, ok, MEAN, p, 1439, 0)
        refused("out_bytes is 481, the band takes exactly 480 (6 rows of 20 pixels, 4 bytes each)", name, whole._h, 8, ok, RGBA8, p, 481, HOST | MIRROR)
        refused("out_bytes is 0, the band takes exactly 360 (6 rows of 20 pixels, 3 bytes each)", name, whole._h, 8, ok, RGB8, None, 0, HOST)
        refused("out_bytes is 3, the band takes exactly 0 (0 rows of 20 pixels, 3 bytes each)", name, empty._h, 8, ok, RGB8, None, 3, 0)
        refused("null output pointer", name, whole._h, 8, ok, RGB8, None, 360, HOST)
        refused("null output pointer", name, whole._h, 8, ok, MEAN, None, 1440, 0)        # (null is aligned: the pointer's own message)
        refused(ALIGNED, name, whole._h, 8, ok, MEAN, p + 1, 1440, 0)
        refused(ALIGNED, name, whole._h, 8, ok, MEAN, p + 2, 1440, MIRROR)
        refused(ALIGNED, name, whole._h, 8, ok, RGBA8, p + 3, 480, 0)
        for fmt in (MEAN, RGB8, RGBA8):                                                    # an empty band: nothing to do, whatever the pointer
            assert call(name, empty._h, 8, ok, fmt, None, 0, 0) == 0, name
            assert call(name, empty._h, 8, ok, fmt, p + 1, 0, HOST | MIRROR) == 0, name
        # ---- a striped handle: the filters refuse it in front of out_bytes and the pointer, amber_hip_pt_resolve takes it
        if name == RESOLVE:
            refused("out_bytes is 360, the band takes exactly 180 (3 rows of 20 pixels, 3 bytes each)", name, striped._h, 8, ok, RGB8, p, 360, HOST)
            refused("null output pointer", name, striped._h, 8, ok, RGB8, None, 180, HOST)
            continue
        refused(STRIPED, name, striped._h, 8, ok, RGB8, p, 180, HOST)
        refused(STRIPED, name, striped._h, 8, ok, RGB8, None, 180, HOST)                  # striped and a null pointer: striped
        refused(STRIPED, name, striped._h, 8, ok, MEAN, p + 1, 7, 0)
        refused("unknown flag bits", name, striped._h, 8, ok, RGB8, p, 180, 4)
        # ---- the parameters, in front of every output argument
        _, k4, n_reserved, lowest = FILTERS[name]
        bad_output = (3, None, 1, 4)
        refused("null params", name, whole._h, 8, None, RGB8, p, 360, HOST)
        refused("null params", name, whole._h, 0, None, *bad_output)
        refused("n_samples is 0", name, whole._h, 0, params(name, levels=9), *bad_output)
        refused(f"levels is 9, not {lowest} .. 8", name, whole._h, 8, params(name, levels=9), RGB8, p, 360, HOST)
        refused(f"levels is 4294967295, not {lowest} .. 8", name, whole._h, 8, params(name, levels=0xffffffff, k_normal=-1.0), *bad_output)
        if lowest == 1:
            refused("levels is 0, not 1 .. 8", name, whole._h, 8, params(name, levels=0), RGB8, p, 360, HOST)
        for i, field in enumerate(("k_normal", "k_albedo", "k_depth", k4)):
            for bad in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
                refused(field + " is negative, NaN or infinite", name, whole._h, 8, params(name, **{field: bad}), RGB8, p, 360, HOST)
            later = {f: float("nan") for f in ("k_normal", "k_albedo", "k_depth", k4)[i:]}   # several bad constants: the first one in this order
            refused(field + " is negative, NaN or infinite", name, striped._h, 8, params(name, reserved=(1,) * n_reserved, **later), *bad_output)
        for word in range(n_reserved):
            reserved = tuple(int(j == word) << (15 * word) for j in range(n_reserved))      # one bit, in this word only
            refused("reserved fields must be 0", name, whole._h, 8, params(name, reserved=reserved), RGB8, p, 360, HOST)
            refused("reserved fields must be 0", name, striped._h, 8, params(name, reserved=reserved), *bad_output)
        if name == "amber_hip_pt_denoise_variance":                                       # behind the constants, in front of the reserved words
            refused("var_radius is 4, not 0 .. 3", name, whole._h, 8, params(name, var_radius=4), RGB8, p, 360, HOST)
            refused("var_radius is 4294967295, not 0 .. 3", name, whole._h, 8, params(name, var_radius=0xffffffff, reserved=(1, 1)), *bad_output)
            refused("k_lum is negative, NaN or infinite", name, whole._h, 8, params(name, var_radius=4, k_lum=-1.0), RGB8, p, 360, HOST)
        if name == "amber_hip_pt_temporal":                                               # behind levels, in front of the constants
            refused("max_history is 0, not 1 .. 65535", name, whole._h, 8, params(name, max_history=0), RGB8, p, 360, HOST)
            refused("max_history is 65536, not 1 .. 65535", name, whole._h, 8, params(name, max_history=65536, k_normal=-1.0, reserved=(1, 1)), *bad_output)
            refused("levels is 9, not 0 .. 8", name, whole._h, 8, params(name, levels=9, max_history=0), RGB8, p, 360, HOST)
    assert (buf == 0xAB).all()

    # ---- the nine companions (and amber_hip_pt_aov_pass): a null handle, a null pointer
    dptr, n_pixels = ctypes.c_void_p(), ctypes.c_uint64()
    where = (ctypes.byref(dptr), ctypes.byref(n_pixels))
    for kind, reset in (("aov", "amber_hip_pt_aov_clear"), ("moments", "amber_hip_pt_moments_clear"), ("history", "amber_hip_pt_temporal_reset")):
        download, device = f"amber_hip_pt_{kind}_download", f"amber_hip_pt_device_{kind}"
        for handle in (whole, striped, empty):
            for name, tail, args in ((reset, "null handle", (None,)),
                                     (download, "null handle or output pointer", (None, p)), (download, "null handle or output pointer", (None, None)),
                                     (download, "null handle or output pointer", (handle._h, None)),
                                     (device, "null handle or pointer", (None,) + where), (device, "null handle or pointer", (None, None, None)),
                                     (device, "null handle or pointer", (handle._h, None, ctypes.byref(n_pixels)))):
                assert getattr(lib, name)(*args) == EINVAL, (name, args)
                assert lib.amber_hip_last_error() == (name + ": " + tail).encode(), (name, args)
    assert lib.amber_hip_pt_aov_pass(None, 0, 8) == EINVAL and lib.amber_hip_last_error() == b"amber_hip_pt_aov_pass: null handle"
    assert lib.amber_hip_pt_aov_pass(whole._h, 0xffffffff, 1) == EINVAL and lib.amber_hip_last_error() == b"amber_hip_pt_aov_pass: sample index overflow"
    assert dptr.value is None and n_pixels.value == 0 and (buf == 0xAB).all()
    for handle in (whole, striped, empty):
        handle.close()

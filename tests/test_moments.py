"""amber_hip_pt_render_batch and the moments buffer on the GPU (amber_amd/csrc/hip/denoise_variance.inc: moments_fold_kernel; pt_host.hip: the accumulation
target).  Every comparison of floats is exact equality of bits: the framebuffer against render_pass on a twin handle (short batches) or against
fb + B in numpy (a long batch), the moments against tests/denoise_variance_reference.py's moments_update over the batches' own sums B, which a third,
cleared handle renders.

The scene is a small room whose ceiling and back wall emit, with three spheres, a disk and a cylinder (17 objects with the aperture blades): at
64 x 48 the CPU oracle finds light in 72 % of the pixels in a batch of one sample and in more for longer ones, so the sums compared here are not
zeros (asserted: at least half of the band's pixels in every batch).  On the Cornell box almost every batch sum is 0 and the test would pass vacuously."""
import os

import numpy as np
import pytest

import denoise_variance_reference as V

pytestmark = pytest.mark.gpu
F32 = np.float32
W, H, SEED = 64, 48, 5
SHORT = ((0, 1), (1, 1), (2, 3), (5, 8))                                             # each at most one accumulation chunk
LONG = (13, 20)                                                                     # three chunks: summed first, added once


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def light_room():
    objects = [(0, 0, [-2, 1.6, -2, 2, 1.6, -2, 2, 1.6, 2]), (0, 0, [-2, 1.6, -2, 2, 1.6, 2, -2, 1.6, 2]),              # ceiling, facing down: emits
               (0, 4, [-2, -1, -2, 2, 1.6, -2, -2, 1.6, -2]), (0, 4, [-2, -1, -2, 2, -1, -2, 2, 1.6, -2]),              # back wall, facing the lens: emits
               (0, 1, [-2, -1, -2, 2, -1, 2, 2, -1, -2]), (0, 1, [-2, -1, -2, -2, -1, 2, 2, -1, 2]),                    # floor
               (1, 2, [0.7, -0.5, 0.1, 0.5]), (1, 3, [-0.8, -0.55, 0.3, 0.45]), (1, 1, [0.0, 0.8, -0.2, 0.3]),
               (2, 1, [-1.8, 0.2, 0.0, 1.0, 0.0, 0.0, 0.8]), (3, 1, [1.4, -1.0, -1.0, 0.0, 1.0, 0.0, 0.2, 1.1])]
    params = np.zeros((len(objects), 12), F32)
    for i, (_, _, p) in enumerate(objects):
        params[i, :len(p)] = p
    return dict(kinds=np.array([o[0] for o in objects], np.uint32), material_index=np.array([o[1] for o in objects], np.uint32), params=params,
                materials=[(4, (3.0, 2.0, 1.0), 0.0), (0, (0.7, 0.7, 0.7), 0.0), (2, (0.9, 0.9, 0.9), 0.0), (3, (1.0, 1.0, 1.0), 1.5), (4, (0.5, 1.5, 2.5), 0.0)],
                transform=[1, 0, 0, 0, 0, 1, 0, 0.1, 0, 0, 1, 3.2, 0, 0, 0, 1], focal_length=0.05, focus_distance=3.2, radius=0.02, n_blades=6)


@pytest.fixture(scope="module")
def room(amber):
    return amber.HostScene.create_arrays(**light_room())


def tracer(amber, room, engine=0, flags=0, **kw):
    return amber.PathTracer(room, amber.Sensor.default(W, H), seed=SEED, engine=engine, flags=flags, **kw)


def batch_sums(alone, first, n):
    """B: what render_pass(first, n) leaves in a framebuffer that held +0, and its rays"""
    alone.clear()
    alone.render_pass(first, n)
    b, rays = alone.download()
    lit = b.any(axis=-1).mean() if b.size else 1.0
    assert lit >= 0.5, (first, n, f"only {lit:.3f} of the band's pixels carry light")
    return b, rays


ENGINES = {"AUTO": (0, 0), "LIST": (1, 0), "BVH": (3, 0), "BVH + BVH_ITEMS": (3, 4), "BVH + DEVICE_BUILD": (3, 8), "BVH + BVH_ITEMS + DEVICE_BUILD": (3, 12),
           "REFERENCE_BVH": (6, 0)}


@pytest.mark.parametrize("engine", list(ENGINES))
def test_batches_against_passes(amber, room, engine):
    eng, flags = ENGINES[engine]
    assert (amber.ENGINE_LIST, amber.ENGINE_BVH, amber.ENGINE_REFERENCE_BVH, amber.PT_FLAG_BVH_ITEMS, amber.PT_FLAG_DEVICE_BUILD) == (1, 3, 6, 4, 8)
    batched, passed, alone = (tracer(amber, room, eng, flags) for _ in range(3))
    # (a) short batches: the framebuffer and the ray count are render_pass's, after every batch; (c) the moments
    moments = np.zeros((H, W, 4), F32)
    for first, n in SHORT:
        batched.render_batch(first, n)
        passed.render_pass(first, n)
        (got, got_rays), (want, want_rays) = batched.download(), passed.download()
        assert np.array_equal(bits(got), bits(want)) and got_rays == want_rays and got_rays > 0, (first, n)
        moments = V.moments_update(moments, batch_sums(alone, first, n)[0], n)
    got_m = batched.moments_download()
    assert got_m.dtype == F32 and got_m.shape == (H, W, 4)
    assert np.array_equal(bits(got_m), bits(moments)) and (got_m[..., 2] == len(SHORT)).all() and not got_m[..., 3].any() and (got_m[..., 1] > 0).mean() >= 0.5
    assert not passed.moments_download().any()                                       # render_pass leaves the moments alone
    # (b) one long batch: summed first, added once
    before, rays_before = batched.download()
    b, b_rays = batch_sums(alone, *LONG)
    batched.render_batch(*LONG)
    got, got_rays = batched.download()
    assert np.array_equal(bits(got), bits(before + b)) and got_rays == rays_before + b_rays
    passed.render_pass(*LONG)
    assert not np.array_equal(bits(got), bits(passed.download()[0]))                  # ... which is not render_pass's order (chunk by chunk onto the pixel)
    moments = V.moments_update(moments, b, LONG[1])
    assert np.array_equal(bits(batched.moments_download()), bits(moments))
    # (d) the two buffers are cleared apart; n_samples == 0 changes nothing; render_pass afterwards behaves as before
    batched.render_batch(40, 0)
    assert np.array_equal(bits(batched.moments_download()), bits(moments)) and np.array_equal(bits(batched.download()[0]), bits(got))
    batched.clear()
    assert not batched.download()[0].any() and batched.download()[1] == 0 and np.array_equal(bits(batched.moments_download()), bits(moments))
    passed.clear()
    batched.render_pass(33, 11)
    passed.render_pass(33, 11)
    (got, got_rays), (want, want_rays) = batched.download(), passed.download()
    assert np.array_equal(bits(got), bits(want)) and got_rays == want_rays and got.any()
    assert np.array_equal(bits(batched.moments_download()), bits(moments))
    batched.moments_clear()
    assert not batched.moments_download().any() and np.array_equal(bits(batched.download()[0]), bits(want))
    batched.render_batch(44, 2)                                                       # and the moments start again from zero
    assert np.array_equal(bits(batched.moments_download()), bits(V.moments_update(np.zeros((H, W, 4), F32), batch_sums(alone, 44, 2)[0], 2)))
    ptr, n_pixels = batched.device_moments()
    assert ptr and n_pixels == W * H
    for pt in (batched, passed, alone):
        pt.close()


def test_a_launch_inside_a_batch_that_runs_out_of_record_slots_is_repeated_into_the_batch(amber, room):
    """AMBER_TEST_RECORD_DENSITY_SCALE, the lab's record-slot hook (read once, at create), makes the handle believe that paths leave 50 times fewer
    records than they do: the second launch gets the probe's buffer, runs out of slots and is repeated by the host.  Inside a batch the repeat must
    add to the batch buffer; a repeat of a render_pass that is still unchecked when a batch begins must add to the framebuffer."""
    plain, alone = tracer(amber, room), tracer(amber, room)
    os.environ["AMBER_TEST_RECORD_DENSITY_SCALE"] = "0.02"
    try:
        hooked = tracer(amber, room)
    finally:
        os.environ.pop("AMBER_TEST_RECORD_DENSITY_SCALE", None)
    moments = np.zeros((H, W, 4), F32)
    for first, n in ((0, 1), (1, 8)):                                                 # the probe (a slot for every path), then eight times its paths in its buffer
        hooked.render_batch(first, n)
        plain.render_batch(first, n)
        moments = V.moments_update(moments, batch_sums(alone, first, n)[0], n)
    assert hooked.kernel_time()[0] >= 3 and plain.kernel_time()[0] == 2               # probe, the launch that ran out, its repetition
    (got, got_rays), (want, want_rays) = hooked.download(), plain.download()
    assert np.array_equal(bits(got), bits(want)) and got_rays == want_rays
    assert np.array_equal(bits(hooked.moments_download()), bits(moments)) and np.array_equal(bits(plain.moments_download()), bits(moments))
    hooked.close()
    os.environ["AMBER_TEST_RECORD_DENSITY_SCALE"] = "0.02"
    try:
        hooked = tracer(amber, room)
    finally:
        os.environ.pop("AMBER_TEST_RECORD_DENSITY_SCALE", None)
    plain.clear()
    plain.moments_clear()
    for pt in (hooked, plain):
        pt.render_pass(0, 1)
        pt.render_pass(1, 8)                                                          # runs out of slots; nobody has looked when the batch begins
        pt.render_batch(9, 1)
    assert hooked.kernel_time()[0] >= 4                                               # probe, the launch that ran out, its repetition, the batch
    (got, got_rays), (want, want_rays) = hooked.download(), plain.download()
    assert np.array_equal(bits(got), bits(want)) and got_rays == want_rays
    moments = V.moments_update(np.zeros((H, W, 4), F32), batch_sums(alone, 9, 1)[0], 1)
    assert np.array_equal(bits(hooked.moments_download()), bits(moments)) and np.array_equal(bits(plain.moments_download()), bits(moments))
    for pt in (hooked, plain, alone):
        pt.close()


def test_a_band_and_an_empty_band(amber, room):
    rows = (5, 29)
    batched, passed, alone = (tracer(amber, room, rows=rows) for _ in range(3))
    moments = np.zeros((rows[1] - rows[0], W, 4), F32)
    for first, n in SHORT:
        batched.render_batch(first, n)
        passed.render_pass(first, n)
        moments = V.moments_update(moments, batch_sums(alone, first, n)[0], n)
    (got, got_rays), (want, want_rays) = batched.download(), passed.download()
    assert got.shape == (24, W, 3) and np.array_equal(bits(got), bits(want)) and got_rays == want_rays
    assert np.array_equal(bits(batched.moments_download()), bits(moments)) and batched.device_moments()[1] == 24 * W
    whole = tracer(amber, room)
    for first, n in SHORT:
        whole.render_batch(first, n)
    assert np.array_equal(bits(whole.moments_download()[rows[0]:rows[1]]), bits(moments))      # a band's pixels are the frame's
    for pt in (batched, passed, alone, whole):
        pt.close()
    empty = tracer(amber, room, rows=(5, 5))
    empty.render_batch(0, 4)
    empty.moments_clear()
    assert empty.moments_download().shape == (0, W, 4) and empty.device_moments() == (None, 0) and empty.download()[1] == 0
    empty.close()

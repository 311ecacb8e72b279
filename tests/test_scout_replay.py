"""The scout and its replay (csrc/hip/pt_megakernel.inc AMBER_KERNEL_SCOUT, pt_replay.inc, scout_bound.h) against the full kernel.

A handle of the 32-object two-phase engine traces every path without its weight and traces again, with weights, the paths the scout flagged; with
AMBER_PT_FLAG_NO_SCOUT every path carries its weight, as before.  Both must give the same framebuffer bits and the same ray count on every scene, however
the samples are split into passes, bands and batches; the scout's flags (amber_hip_kat_scout_flags: the bitmap after the scout, before the replay) must
cover every path whose measurement is not +0 (amber_hip_pt_trace_paths from the path's own eye ray), and be exactly those on scenes without degenerate
weights.

Scenes: the Cornell box; LIT_BOX, a 20-object room under a ceiling light 1.6 wide (a third of its paths end on the light); HOT_BOX, the same room with scatter
weights of 3e30, 1e-30 and negative ones, whose path weights overflow to inf and carry NaN measurements across bounces (the case seed 520075 of
test_gpu_parity.test_fuzz_regressions stands for: that scene has 292 objects and cannot render through the 32-object engine); and the seeds of that test
with at most 32 objects, under their --scaled / --extreme switches, 31296 among them.

amber_hip_pt_update_lens and amber_hip_pt_update_objects refuse every handle that is not engine BVH's, so a scouting handle never sees a new lens or a
moved object: the last test pins that the refusal stands and leaves the handle rendering the same bits."""
import os

import numpy as np
import pytest

from f64_reference import xorshift_uniform
from fuzz_scenes import scene_for_seed

pytestmark = pytest.mark.gpu
F32 = np.float32
W, H, SEED = 48, 40, 7
FUZZ = ((5, 0, 0), (1037, 0, 0), (2, 0, 0), (16, 0, 0), (40, 0, 0), (31296, 0, 1), (209769, 1, 1), (308053, 1, 0))   # (seed, scaled, extreme): <= 32 objects


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _box(wall_rho, mirror_rho):
    c8 = [(-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)]
    objects = []
    for a, b, c, d, m in ((0, 1, 2, 3, 1), (0, 4, 5, 1, 1), (3, 2, 6, 7, 1), (0, 3, 7, 4, 2), (1, 5, 6, 2, 3)):       # back, floor, ceiling, left, right
        objects += [(0, m, [*c8[a], *c8[b], *c8[c]]), (0, m, [*c8[c], *c8[d], *c8[a]])]
    L = [(-0.8, 0.99, -0.8), (0.8, 0.99, -0.8), (0.8, 0.99, 0.8), (-0.8, 0.99, 0.8)]                                   # the light: faces down
    objects += [(0, 0, [*L[0], *L[1], *L[2]]), (0, 0, [*L[2], *L[3], *L[0]])]
    objects += [(1, 4, [-0.45, -0.6, -0.3, 0.4]), (1, 5, [0.5, -0.65, 0.3, 0.35])]                                    # a mirror and a glass sphere
    materials = [(4, (20.0, 15.0, 10.0), 0.0), (0, wall_rho, 0.0), (0, (0.75, 0.25, 0.25), 0.0), (0, (0.25, 0.75, 0.25), 0.0), (2, mirror_rho, 0.0),
                 (3, (1.0, 1.0, 1.0), 1.5)]
    return dict(objects=objects, materials=materials, transform=[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 4, 0, 0, 0, 1], focal_length=0.05, focus_distance=4.0,
                radius=0.02, n_blades=6)


LIT_BOX = _box((0.75, 0.75, 0.75), (0.9, 0.9, 0.9))
HOT_BOX = _box((3e30, 1e-30, -2.0), (1e25, 0.5, -1e-20))


@pytest.fixture(scope="module")
def scenes(amber):
    """name -> (host scene, draws of its eye-ray generator, degenerate weights expected)"""
    out = {"cornell": (amber.HostScene.cornell_box(), 5, False), "lit": (amber.HostScene.create(**LIT_BOX), 5, False),
           "hot": (amber.HostScene.create(**HOT_BOX), 5, True)}
    for seed, scaled, extreme in FUZZ:
        sc, _ = scene_for_seed(seed, scaled=bool(scaled), extreme=bool(extreme))
        assert len(sc["objects"]) + max(1, sc["n_blades"]) <= 32
        out[f"fuzz{seed}"] = (amber.HostScene.create(**sc), 5 if sc["n_blades"] else 2, True)
    return out


NAMES = ["cornell", "lit", "hot"] + [f"fuzz{s}" for s, _, _ in FUZZ]


def pair(amber, hs, w=W, h=H, **kw):
    """(scouting handle, full-kernel handle) of the 32-object two-phase engine"""
    sn = amber.Sensor.default(w, h)
    return (amber.PathTracer(hs, sn, seed=SEED, engine=amber.ENGINE_TWO_PHASE, **kw),
            amber.PathTracer(hs, sn, seed=SEED, engine=amber.ENGINE_TWO_PHASE, flags=amber.api.PT_FLAG_NO_SCOUT, **kw))


def same(scout, full):
    (a, ra), (b, rb) = scout.download(), full.download()
    return ra == rb and np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("name", NAMES)
def test_scout_on_equals_scout_off(amber, scenes, name):
    """One pass of 64 samples, split passes (0..7, 7..40, 40..64), 33 samples (not a multiple of 32), max_depth 2 and 16, interleaved stripes, and batches into
    the moments buffer: framebuffer bits, ray counts and moments are those of the full kernel."""
    hs = scenes[name][0]
    for kw, passes in ((dict(), ((0, 64),)), (dict(), ((0, 7), (7, 33), (40, 24))), (dict(), ((3, 33),)), (dict(max_depth=2), ((0, 16),)),
                       (dict(max_depth=16), ((0, 16),)), (dict(rows=(3, H - 2), stripe=(2, 6)), ((0, 7), (7, 33)))):
        scout, full = pair(amber, hs, **kw)
        for first, n in passes:
            scout.render_pass(first, n); full.render_pass(first, n)
        assert same(scout, full), (name, kw, passes)
        assert scout.kernel_time()[0] == full.kernel_time()[0] == len(passes)          # the replay is part of its launch: one launch per pass
        scout.close(); full.close()
    scout, full = pair(amber, hs)
    for first, n in ((0, 4), (4, 1), (5, 11)):
        scout.render_batch(first, n); full.render_batch(first, n)
    assert same(scout, full) and np.array_equal(bits(scout.moments_download()), bits(full.moments_download())), name
    scout.close(); full.close()


def _measured(amber, pt, draws, n_samples):
    """The measurement of every path q = pixel * n_samples + sample of one launch over samples [0, n_samples): amber_hip_pt_trace_paths from the path's own eye
    ray (origin, direction, weight and sampler state as the render kernels hold them at the first cast) -- and that eye weight itself."""
    pixel = np.repeat(np.arange(W * H, dtype=np.uint32), n_samples)
    sample = np.tile(np.arange(n_samples, dtype=np.uint32), W * H)
    eye = pt.kat_eye(pixel, sample)
    states = np.array(amber.sampler_states(SEED, pixel, sample), np.uint64, copy=True)
    for _ in range(draws):
        xorshift_uniform(states)
    rgb, _, _ = pt.trace_paths(eye[:, 0:3].copy(), eye[:, 3:6].copy(), np.repeat(eye[:, 6:7], 3, axis=1), states, n_samples=1)
    return rgb, eye[:, 6]


@pytest.mark.parametrize("name", NAMES)
def test_the_flags_cover_every_path_with_a_measurement(amber, scenes, name):
    """Conservative everywhere, exact where no weight degenerates.  On the two ordinary scenes equality also says that no path is flagged as suspect alone: a
    path flagged only for its bound would have to have a measurement -- of which there are at least 100 on the lit scene, so nothing passes vacuously.
    Every scene here lies inside the ranges of scout_bound.h, so every one must scout: a handle that fell back would compare the full kernel with itself.
    The host's bound of the eye weight is held against the real generator too: the weight amber_hip_kat_eye's GenerateEyeRay gives every path is at most
    2^(bound0 / 16), or the scout's guard has flagged the path."""
    hs, draws, degenerate = scenes[name]
    n = 64 if name == "cornell" else 16
    scout, full = pair(amber, hs)
    flagged, scouts = scout.kat_scout_flags(0, n)
    assert not full.kat_scout_flags(0, n)[1]
    assert scouts, name
    rgb, eye_weight = _measured(amber, full, draws, n)
    within = np.abs(eye_weight.astype(np.float64)) <= 2.0 ** (scout.scout_bound0 / 16.0)          # False for a NaN weight
    print(f"\n{name}: bound0 {scout.scout_bound0 / 16.0:.2f} bits, largest |eye weight| 2^{np.log2(np.nanmax(np.abs(eye_weight.astype(np.float64))) + 1e-300):.2f}")
    assert (within | flagged).all(), (name, int((~within & ~flagged).sum()))
    assert within.mean() > 0.99, name                                   # ... and the guard is no excuse: nearly every ray is inside the bound
    measured = bits(rgb).any(axis=1)                                    # anything but (+0, +0, +0)
    print(f"{name}: {int(flagged.sum())} of {flagged.size} paths flagged, {int(measured.sum())} with a measurement")
    assert not (measured & ~flagged).any(), (name, int((measured & ~flagged).sum()))
    if not degenerate:
        assert np.array_equal(flagged, measured), name
    if name == "lit":
        assert measured.sum() >= 100
    if name == "hot":
        assert (~np.isfinite(rgb)).any(axis=1).sum() >= 100                # the overflowing weights are what this scene is for: inf and NaN measurements
    scout.render_pass(0, n); full.render_pass(0, n)                       # the handle renders as ever after the lab call left the bitmap dirty
    assert same(scout, full)
    scout.close(); full.close()


def test_a_scouted_launch_that_runs_out_of_record_slots_is_repeated(amber, scenes):
    """AMBER_TEST_RECORD_DENSITY_SCALE (read once, at create) makes the handle believe that paths leave 50 times fewer records than they do: the second launch
    gets the probe's buffer, the scout runs out of slots, the replay and the reduction leave no trace, and the host repeats scout and replay."""
    hs = scenes["lit"][0]
    os.environ["AMBER_TEST_RECORD_DENSITY_SCALE"] = "0.02"
    try:
        scout, full = pair(amber, hs, 64, 64)
    finally:
        os.environ.pop("AMBER_TEST_RECORD_DENSITY_SCALE", None)
    plain, _unused = pair(amber, hs, 64, 64)
    for pt in (scout, full, plain):
        pt.render_pass(0, 1)
        pt.render_pass(1, 8)
    assert scout.kernel_time()[0] >= 3 and full.kernel_time()[0] >= 3 and plain.kernel_time()[0] == 2      # probe, the launch that ran out, its repetition
    assert same(scout, full) and same(scout, plain)
    for pt in (scout, full, plain, _unused):
        pt.close()


def test_a_lens_the_host_cannot_bound_renders_with_the_full_kernel(amber):
    """A focus distance of 4e7 is outside the ranges for which scout_bound.h bounds the eye weight (lengths up to 2^20).  The handle must say that it does not
    scout, and equal engine LIST."""
    sc = dict(LIT_BOX, focus_distance=4.0e7)
    hs = amber.HostScene.create(**sc)
    sn = amber.Sensor.default(W, H)
    pt = amber.PathTracer(hs, sn, seed=SEED, engine=amber.ENGINE_TWO_PHASE)
    flagged, scouts = pt.kat_scout_flags(0, 4)
    assert not scouts and not flagged.any()
    lst = amber.PathTracer(hs, sn, seed=SEED, engine=amber.ENGINE_LIST)
    pt.render_pass(0, 16); lst.render_pass(0, 16)
    assert same(pt, lst)
    pt.close(); lst.close()


def test_updates_stay_refused_on_scouting_handles(amber, scenes):
    """The decision to scout is made at create; nothing can invalidate it later, because the two calls that change a live handle's lens or objects take engine
    BVH's handles only.  They must keep refusing this one, and leave it rendering the same bits."""
    hs = scenes["lit"][0]
    scout, full = pair(amber, hs)
    scout.render_pass(0, 8); full.render_pass(0, 8)
    with pytest.raises(amber.AmberError):
        scout.update_lens(amber.HostScene.create(**dict(LIT_BOX, focus_distance=3.0)))
    objs, _, _ = hs.flatten()
    with pytest.raises(amber.AmberError):
        scout.update_flat(0, np.frombuffer(objs, dtype=amber.api._RECORD)[:1].copy(), amber.UPDATE_REFIT)
    scout.render_pass(8, 8); full.render_pass(8, 8)
    assert same(scout, full)
    scout.close(); full.close()

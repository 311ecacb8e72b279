"""amber_hip_lt_render_pass: light-tracing passes accumulated into the handle's framebuffer on the device must leave the bits that adding
amber_hip_lt_trace's records in the reference's order leaves (tests/lt_accumulate_reference.py restates that order from the header's text), for real
records on every engine, for any split of the passes, on a framebuffer that already holds something, through a launch that ran out of record slots,
and -- through the lab hook amber_hip_kat_lt_accumulate -- for synthetic record lists that put the ordering and the ordered sum under load.

The `lights` scene is test_light_tracing's (wide aperture) at 48 x 36.  Its sensor is enlarged until the light that comes through the aperture lands on
it: the record count then saturates near 15 per pass (950 in 64 passes, whatever the sensor's size -- the aperture, not the sensor, bounds it), so the
2 000 records the real-record cases ask for take N_PASSES = 192 passes, not 64; the splitting and output-stage cases run over 64 passes."""
import numpy as np
import pytest

import lt_accumulate_reference as R

pytestmark = pytest.mark.gpu

W, H = 48, 36
N_PASSES = 192
SEED = 13
LIGHTS = dict(
    materials=[(4, (30.0, 20.0, 10.0), 0.0), (0, (0.7, 0.6, 0.5), 0.0), (2, (0.8, 0.8, 0.8), 0.0), (3, (1.0, 1.0, 1.0), 1.5), (4, (5.0, 5.0, 9.0), 0.0)],
    objects=[
        (2, 0, [0.0, 1.5, 0.0, 0.0, -1.0, 0.0, 0.6]),                      # disk light
        (0, 4, [-1.0, 1.4, -1.0, -1.0, 1.4, 1.0, -0.5, 1.4, 0.0]),        # triangle light
        (1, 0, [1.2, 0.8, 0.0, 0.15]),                                     # sphere light
        (3, 4, [-1.4, -0.5, 0.5, 0.0, 1.0, 0.0, 0.1, 0.6]),               # cylinder light
        (0, 1, [-3, -1, -3, 3, -1, 3, 3, -1, -3]), (0, 1, [-3, -1, -3, -3, -1, 3, 3, -1, 3]),
        (1, 2, [0.7, -0.6, -0.3, 0.4]), (1, 3, [0.0, -0.5, 0.8, 0.45]),
    ],
    transform=[1, 0, 0, 0, 0, 1, 0, 0.2, 0, 0, 1, 2.6, 0, 0, 0, 1], focal_length=0.05, focus_distance=2.6, radius=0.45, n_blades=5,
)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def sensor_of(amber, width, height, scale):
    return amber.Sensor(width, height, np.float32(0.036 * scale), np.float32(0.036 / width * height * scale))


class Real:
    """The lights scene, the sensor that catches enough of its light, lt_trace's records and the restatement's image of them: computed once."""

    def __init__(self, amber):
        self.amber = amber
        self.hs = amber.HostScene.create(**LIGHTS)
        for self.scale in (1, 2, 4, 8, 16, 32, 64):
            pt = self.tracer()
            self.rec, self.rays = pt.lt_trace(0, N_PASSES)
            pt.close()
            if len(self.rec) >= 2000:
                break
        self.rec.setflags(write=False)
        self.image = R.accumulate(self.rec, W, H)
        self.image.setflags(write=False)
        first = self.rec[self.rec["sample"] < 64]
        pt = self.tracer()
        self.rays64 = pt.lt_trace(0, 64)[1]
        pt.close()
        self.image64 = R.accumulate(first, W, H)
        self.image64.setflags(write=False)

    def sensor(self):
        return sensor_of(self.amber, W, H, self.scale)

    def tracer(self, **kw):
        return self.amber.PathTracer(self.hs, self.sensor(), seed=SEED, **kw)


@pytest.fixture(scope="module")
def real(amber):
    return Real(amber)


def test_the_scene_gives_the_records_the_cases_need(real):
    rec = real.rec
    assert len(rec) >= 2000, (real.scale, len(rec))
    key = (rec["pixel"].astype(np.uint64) << np.uint64(32)) | rec["sample"]
    assert np.unique(key, return_counts=True)[1].max() >= 2                       # some pixel receives two records in one pass
    assert max(len(np.unique(rec["sample"][rec["pixel"] == p])) for p in np.unique(rec["pixel"])) >= 2   # ... and some pixel records in two passes
    order = np.lexsort((rec["bounce"], rec["path"], rec["sample"]))
    assert np.array_equal(order, np.arange(len(rec)))                             # the list is in (pass, path, bounce) order
    assert not np.array_equal(bits(real.image), bits(R.accumulate(rec[rec["sample"] < 64], W, H))) and real.image.any()


ENGINES = [("auto", "ENGINE_AUTO", 0), ("list", "ENGINE_LIST", 0), ("two_phase", "ENGINE_TWO_PHASE", 0), ("bvh", "ENGINE_BVH", 0),
           ("bvh_items", "ENGINE_BVH", "PT_FLAG_BVH_ITEMS"), ("reference_bvh", "ENGINE_REFERENCE_BVH", 0)]


@pytest.mark.parametrize("label,engine,flags", ENGINES, ids=[e[0] for e in ENGINES])
def test_real_records_on_every_engine(amber, real, label, engine, flags):
    pt = real.tracer(engine=getattr(amber, engine), flags=getattr(amber, flags) if flags else 0)
    assert len(real.rec) >= 2000
    info = pt.lt_render_pass(0, N_PASSES)
    img, rays = pt.download()
    assert rays == real.rays == info["n_rays"] and info["n_splats"] == len(real.rec) and info["n_repeats"] == 0 and info["n_launches"] >= 1
    assert info["longest_run"] == R.longest_run(real.rec) >= 2
    assert np.array_equal(bits(img), bits(real.image))
    assert pt.kernel_time()[0] == info["n_launches"]
    pt.close()


def test_the_cornell_box_splats_rarely_or_never(amber):
    hc = amber.HostScene.cornell_box()
    sensor = amber.Sensor.default(64, 64)
    rec, rays = amber.PathTracer(hc, sensor, seed=3).lt_trace(0, 48)
    pt = amber.PathTracer(hc, sensor, seed=3)
    info = pt.lt_render_pass(0, 48)
    img, got_rays = pt.download()
    assert len(rec) < 200 and info["n_splats"] == len(rec) and got_rays == rays > 0
    assert np.array_equal(bits(img), bits(R.accumulate(rec, 64, 64)))
    touched = np.zeros(64 * 64, bool); touched[rec["pixel"]] = True
    assert not bits(img).reshape(-1, 3)[~touched].any()                           # +0 where nothing landed
    pt.close()


def test_any_split_of_the_passes_leaves_the_same_bits(real):
    whole = real.tracer()
    whole.lt_render_pass(0, 64)
    a, rays_a = whole.download()
    parts = real.tracer()
    parts.lt_render_pass(0, 5)
    parts.lt_render_pass(5, 59)
    b, rays_b = parts.download()
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(real.image64)) and rays_a == rays_b == real.rays64
    one = real.tracer()
    for s in range(0, 64):
        one.lt_render_pass(s, 1)
    c, rays_c = one.download()
    assert np.array_equal(bits(a), bits(c)) and rays_c == rays_a
    for pt in (whole, parts, one):
        pt.close()


def test_it_adds_to_what_the_framebuffer_holds(real):
    pt = real.tracer()
    pt.render_pass(0, 8)
    before, rays_pt = pt.download()
    assert before.any()
    pt.lt_render_pass(0, 64)
    after, rays = pt.download()
    assert np.array_equal(bits(after), bits(R.accumulate(real.rec[real.rec["sample"] < 64], W, H, before))) and rays == rays_pt + real.rays64
    assert not np.array_equal(bits(after), bits(before))
    pt.clear()
    img, rays = pt.download()
    assert rays == 0 and not bits(img).any()
    pt.lt_render_pass(0, 64)                                                       # and the handle goes on as a fresh one would
    assert np.array_equal(bits(pt.download()[0]), bits(real.image64))
    pt.close()


def test_a_launch_that_runs_out_of_slots_is_repeated(amber, real):
    """One launch that produces more records than AMBER_LT_SPLAT_CAPACITY0: the buffer grows, the launch runs again, image and rays stand."""
    width, height = 256, 192
    sensor = sensor_of(amber, width, height, real.scale)
    probe, _ = amber.PathTracer(real.hs, sensor, seed=SEED).lt_trace(0, 16)
    assert len(probe) > 100
    passes = int(np.ceil(1.3 * amber.LT_SPLAT_CAPACITY0 * 16 / len(probe)))        # 30 % over the capacity at the rate lt_trace reports
    assert width * height * passes < 2 ** 31                                       # one launch
    rec, rays = amber.PathTracer(real.hs, sensor, seed=SEED).lt_trace(0, passes, capacity=1 << 18)
    assert len(rec) > amber.LT_SPLAT_CAPACITY0
    want = R.accumulate(rec, width, height)
    pt = amber.PathTracer(real.hs, sensor, seed=SEED)
    info = pt.lt_render_pass(0, passes)
    img, got_rays = pt.download()
    assert info["n_repeats"] >= 1 and info["n_launches"] == 1 + info["n_repeats"] and info["n_splats"] == len(rec)
    assert got_rays == rays == info["n_rays"] and np.array_equal(bits(img), bits(want))
    assert info["longest_run"] == R.longest_run(rec)
    pt.clear()
    again = pt.lt_render_pass(0, passes)                                           # the buffer kept what it grew to
    img, got_rays = pt.download()
    assert again["n_repeats"] == 0 and again["n_launches"] == 1 and got_rays == rays and np.array_equal(bits(img), bits(want))
    pt.close()


def test_the_output_stage_reads_the_frame(amber, real):
    pt = real.tracer()
    pt.lt_render_pass(0, 64)
    fb, _ = pt.download()
    mean = pt.resolve(64, amber.RESOLVE_MEAN_F32)
    assert np.array_equal(bits(mean), bits(fb / np.float32(64))) and mean.any()
    assert np.array_equal(pt.resolve(64, amber.RESOLVE_RGB8), amber.tonemap(fb / np.float32(64)))
    pt.close()


# ---- synthetic records through the hook ------------------------------------------------------------------------------------------------------------
def hook(amber, real, width, height, rec):
    pt = amber.PathTracer(real.hs, sensor_of(amber, width, height, 1), seed=SEED)
    pt.kat_lt_accumulate(rec)
    img, rays = pt.download()
    pt.close()
    assert rays == 0                                                               # the hook traces nothing
    return img


def test_hook_no_record_and_one_record(amber, real):
    empty = np.zeros(0, R.SPLAT_DTYPE)
    assert not bits(hook(amber, real, 5, 3, empty)).any()
    for pixel in (0, 7, 14):
        rec = R.records([3], [9], [2], [pixel], np.float32([[1.5, -2.25, 1e-30]]))
        img = hook(amber, real, 5, 3, rec)
        assert np.array_equal(bits(img), bits(R.accumulate(rec, 5, 3))) and np.count_nonzero(img) == 3


def test_hook_a_long_run_on_one_pixel(amber, real):
    rec = R.one_pixel_fixture(5, 3)                                                # 2^17 records, one pixel, one pass, shuffled
    want = R.accumulate(rec, 5, 3)
    pt = amber.PathTracer(real.hs, sensor_of(amber, 5, 3, 1), seed=SEED)
    pt.kat_lt_accumulate(rec)
    img, _ = pt.download()
    assert np.array_equal(bits(img), bits(want))
    pt.kat_lt_accumulate(rec)                                                      # onto the sum of the first: fb + P, not a longer chain
    twice, _ = pt.download()
    assert np.array_equal(bits(twice), bits(R.accumulate(rec, 5, 3, want)))
    pt.close()


def spread_records(rng):
    """70 000 records over a 5 x 3 frame, pixel 0 and the last pixel included, in 300 passes next to the top of the 32-bit range; bounce 0 and
    0xfffffffe (and a few small values); a third of the paths around width * height - 1, the others anywhere in 32 bits (a (pass, path, bounce) names
    one record, and 300 passes x 2 bounces x a handful of paths do not give 70 000 names)."""
    n = 70000
    pixel = rng.integers(0, 15, n).astype(np.uint32)
    pixel[:2] = (0, 14)
    path = np.where(rng.integers(0, 3, n) == 0, rng.integers(12, 16, n), rng.integers(0, 1 << 32, n)).astype(np.uint32)
    bounce = rng.choice(np.uint32([0, 0xfffffffe, 0, 0xfffffffe, 1, 2, 3]), n)
    sample = (np.uint32(0xfffffe00) + rng.integers(0, 300, n)).astype(np.uint32)
    rgb = (10.0 ** rng.uniform(-5, 5, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))).astype(np.float32)
    rec = R.records(path, sample, bounce, pixel, rgb)
    rec = rec[np.sort(np.unique(np.stack([rec["sample"], rec["path"], rec["bounce"]], 1), axis=0, return_index=True)[1])]
    extra = n - len(rec)                                                           # the clashes, given paths of their own
    more = R.records((1 << 31) + np.arange(extra), rng.choice(rec["sample"], extra), np.zeros(extra), rng.integers(0, 15, extra),
                     (10.0 ** rng.uniform(-5, 5, (extra, 3))).astype(np.float32))
    rec = np.concatenate([rec, more])
    assert len(np.unique(np.stack([rec["sample"], rec["path"], rec["bounce"]], 1), axis=0)) == n
    return rec


def test_hook_many_records_over_a_small_frame(amber, real):
    rng = np.random.default_rng(5)
    rec = spread_records(rng)
    assert len(rec) == 70000 and len(np.unique(rec["sample"])) == 300 and {0, 14} <= set(rec["pixel"].tolist())
    assert {0, 0xfffffffe} <= set(rec["bounce"].tolist()) and R.longest_run(rec) > 8
    want = bits(R.accumulate(rec, 5, 3))
    a = hook(amber, real, 5, 3, rec[rng.permutation(len(rec))])
    b = hook(amber, real, 5, 3, rec[rng.permutation(len(rec))])                    # two shuffles, the same bits
    assert np.array_equal(bits(a), want) and np.array_equal(bits(b), want)


def test_hook_nan_and_inf_stay_on_their_pixels(amber, real):
    rng = np.random.default_rng(6)
    n = 3000
    rgb = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    pixel = rng.integers(0, 12, n).astype(np.uint32)                               # pixels 12, 13, 14 stay empty
    pixel[100], pixel[200], pixel[201] = 5, 5, 6
    rgb[pixel == 3, 0] = np.nan                                                    # NaN given: pixel 3, red
    rgb[100, :] = (np.inf, -np.inf, np.inf)                                        # inf - inf: pixel 5, red
    rgb[200, 0] = -np.inf
    rgb[201, 1] = np.inf
    rec = R.records(np.arange(n), rng.integers(0, 4, n), np.ones(n), pixel, rgb)
    with np.errstate(invalid="ignore"):
        want = R.accumulate(rec, 5, 3).reshape(-1, 3)
    flat = hook(amber, real, 5, 3, rec[rng.permutation(n)]).reshape(-1, 3)
    assert np.array_equal(np.isnan(flat), np.isnan(want))
    assert np.isnan(flat[3, 0]) and np.isnan(flat[5, 0]) and flat[5, 1] == -np.inf and flat[5, 2] == np.inf and flat[6, 1] == np.inf
    clean = np.ones(15, bool); clean[[3, 5, 6]] = False
    assert np.isfinite(flat[clean]).all() and np.isnan(flat).sum() == 2            # NaN stays where it arose
    ok = ~np.isnan(want)
    assert np.array_equal(bits(flat)[ok], bits(want)[ok]) and not bits(flat[12:]).any()


def test_the_adapter_takes_the_new_path(amber, real):
    """`--algorithm lt` through HipLightTracing::Render against the old arithmetic: lt_trace's records added by the restatement, divided by the passes."""
    sensor = real.sensor()
    img, st = real.hs.render(sensor, 150, seed=SEED, samples_per_launch=64, algorithm="lt")
    pt = real.tracer()
    rec, rays = pt.lt_trace(0, 150)
    pt.close()
    want = R.accumulate(rec, W, H) / np.float32(150)
    assert st["passes"] == 150 and st["rays"] == rays and st["launches"] == 3
    assert len(rec) > 1500 and np.array_equal(bits(img), bits(want)) and (img > 0).any()

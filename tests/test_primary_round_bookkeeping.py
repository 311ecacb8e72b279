"""The pixel bookkeeping of a primary round -- path q -> (band pixel, sample) -> (px, py) -- with the host-made exact dividers (exact_div.h)
instead of integer divisions, at the smallest shapes at which it can go wrong.  Cornell box through engines TWO_PHASE and LIST (pt_megakernel):

  * widths 1, 3, 17 and 64 with 8 or 16 rows; 1, 3, 63, 64, 65 and 200 samples per launch, so that the 64 paths of a round straddle pixels and
    the 1024 paths of a claim straddle rows; a nonzero first sample;
  * bands: the stripes stripe_partition(16, 3)[1] deals (and the same with 2-row stripes, so that a band holds several), a contiguous band that
    starts at a nonzero row;
  * one light-tracing launch (lt_trace) at 3 and at 65 passes: its path index / pass bookkeeping divides by the same launch constant;
  * few Cornell paths reach the light at these frame sizes (the images are nearly black: the signatures and ray counts carry the check), so the
    same launches once more on a room whose ceiling and back wall are lights (LIGHT_BOX below): every pixel gets records, and the record
    path (EmitRecords, rec_place_kernel) divides by the sample count too.

Against the oracle (List): image bits and ray count of every launch, and the product kernel's path signatures path by path -- also against the
lab's one-thread-per-path signature kernel, which keeps plain `/` and `%`, where the lab library is loaded; one square frame through
tests/parity_rows.py as the parity tests use it.  Everything equal, no tolerance.  The oracle's results are computed once per shape and shared by
the engines."""
import functools

import numpy as np
import pytest

import oracle_binding as O
from parity_rows import compare_rows

pytestmark = pytest.mark.gpu

SEED = 12345
FRAMES = ((1, 8), (3, 16), (17, 8), (64, 16))
LAUNCHES = ((0, 1), (0, 3), (0, 63), (0, 64), (0, 65), (0, 200), (7, 3), (1000, 65))     # (first sample, samples of the launch)
BAND_FRAMES = ((17, 16), (64, 16))
BAND_LAUNCHES = ((5, 3), (5, 65))
LIGHT_BOX = dict(
    # a room whose ceiling and back wall are lights: most paths end on one
    materials=[(4, (3.0, 2.0, 1.0), 0.0), (0, (0.7, 0.7, 0.7), 0.0), (2, (0.9, 0.9, 0.9), 0.0), (3, (1.0, 1.0, 1.0), 1.5), (4, (0.5, 1.5, 2.5), 0.0)],
    objects=[
        (0, 0, [-2, 1.5, -2, 2, 1.5, -2, 2, 1.5, 2]), (0, 0, [-2, 1.5, -2, 2, 1.5, 2, -2, 1.5, 2]),            # ceiling light (normal -y: facing down)
        (0, 4, [-2, -1, -2, 2, 1.5, -2, -2, 1.5, -2]), (0, 4, [-2, -1, -2, 2, -1, -2, 2, 1.5, -2]),            # back wall light (normal +z)
        (0, 1, [-2, -1, -2, 2, -1, 2, 2, -1, -2]), (0, 1, [-2, -1, -2, -2, -1, 2, 2, -1, 2]),                  # floor
        (1, 2, [0.6, -0.5, 0.0, 0.5]), (1, 3, [-0.7, -0.55, 0.4, 0.45]), (1, 4, [0.0, 0.9, 0.0, 0.3]),
        (2, 0, [-1.9, 0.2, 0.0, 1.0, 0.0, 0.0, 0.9]), (3, 1, [1.5, -1.0, -1.0, 0.0, 1.0, 0.0, 0.2, 1.2]),
    ],
    transform=[1, 0, 0, 0, 0, 1, 0, 0.1, 0, 0, 1, 3.2, 0, 0, 0, 1], focal_length=0.05, focus_distance=3.2, radius=0.02, n_blades=6,
)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _oracle_scene():
    return O.Scene.cornell(O.ACCEL_LIST)


@functools.lru_cache(maxsize=None)
def _oracle(w, h, first, n):
    """Per row of the w x h frame: sums (h, w, 3), casts (h,), path signatures (h, w, n) of one launch of samples [first, first + n)."""
    osc = _oracle_scene()
    img = np.zeros((h, w, 3), np.float32)
    casts = np.zeros(h, np.int64)
    for y in range(h):
        _, cnt = osc.render_xorshift(w, h, SEED, first, n, rows=(y, y + 1), out=img)
        casts[y] = cnt.casts
    sig = osc.path_signatures(w, h, SEED, first, n, (0, h))
    for a in (img, casts, sig):
        a.setflags(write=False)
    return img, casts, sig


def _check_launches(amber, engine, w, h, launches, **band):
    hs = amber.HostScene.cornell_box()
    pt = amber.PathTracer(hs, amber.Sensor.default(w, h), seed=SEED, engine=engine, **band)
    index = np.asarray(pt.row_index)
    for first, n in launches:
        img, casts, sig = _oracle(w, h, first, n)
        pt.clear()
        pt.render_pass(first, n)
        got, rays = pt.download()
        where = (engine, w, h, first, n, band)
        assert rays == int(casts[index].sum()), where
        assert np.array_equal(bits(got), bits(img[index])), where
        sp = pt.render_signatures(first, n)
        assert np.array_equal(sp, sig[index]), where
        if amber.api.is_lab():
            assert np.array_equal(sp, pt.kat_signatures(first, n)), where
    pt.close()


@pytest.fixture(scope="module", params=["two_phase", "list"])
def engine(request, amber):
    return {"two_phase": amber.ENGINE_TWO_PHASE, "list": amber.ENGINE_LIST}[request.param]


def test_whole_frames(amber, engine):
    for w, h in FRAMES:
        _check_launches(amber, engine, w, h, LAUNCHES)


def test_striped_and_offset_bands(amber, engine):
    from amber_amd.distributed import stripe_partition
    for w, h in BAND_FRAMES:
        for part in (stripe_partition(h, 3)[1], stripe_partition(h, 3, stripe_rows=2)[1]):
            assert part["stripe"] is not None
            _check_launches(amber, engine, w, h, BAND_LAUNCHES, rows=part["rows"], stripe=part["stripe"])
        _check_launches(amber, engine, w, h, BAND_LAUNCHES, rows=(3, 11))


def test_a_scene_where_most_paths_leave_a_record(amber, engine):
    from amber_amd.distributed import stripe_partition
    hs, osc = amber.HostScene.create(**LIGHT_BOX), O.Scene.create(**LIGHT_BOX)
    w, h = 17, 16
    part = stripe_partition(h, 3, stripe_rows=2)[1]
    for band in ({}, dict(rows=part["rows"], stripe=part["stripe"])):
        pt = amber.PathTracer(hs, amber.Sensor.default(w, h), seed=SEED, engine=engine, **band)
        index = np.asarray(pt.row_index)
        for first, n in ((0, 1), (7, 3), (0, 65), (3, 200)):
            ref = np.zeros((h, w, 3), np.float32)
            casts = sum(int(osc.render_xorshift(w, h, SEED, first, n, rows=(int(y), int(y) + 1), out=ref)[1].casts) for y in index)
            pt.clear()
            pt.render_pass(first, n)
            got, rays = pt.download()
            assert rays == casts and np.array_equal(bits(got), bits(ref[index])), (engine, first, n, band)
            assert (ref[index].sum(axis=2) > 0).mean() > 0.5        # the records are there: 0.72 of the pixels at one sample, all at 200
        pt.close()


def test_light_tracing_launches(amber, engine):
    """One lt_trace launch at 3 and at 65 passes: ray count and splat records against the oracle."""
    w, h = 64, 16
    pt = amber.PathTracer(amber.HostScene.cornell_box(), amber.Sensor.default(w, h), seed=SEED, engine=engine)
    for first, n in ((0, 3), (2, 65)):
        rec, rays = pt.lt_trace(first, n)
        _, cnt, oref = _oracle_scene().render_lt(w, h, SEED, first, n)
        assert rays == cnt.casts and len(rec) == len(oref), (engine, first, n)
        got = np.stack([rec["path"], rec["sample"], rec["bounce"], rec["pixel"], *[rec["rgb"][:, c].view(np.uint32) for c in range(3)]], 1)
        assert np.array_equal(got.reshape(-1, 7), oref), (engine, first, n)
    pt.close()


def test_a_square_frame_through_the_parity_helper(amber):
    """tests/parity_rows.py as the parity tests call it (the handle's default engine: TWO_PHASE on the Cornell box), 65 samples on two bands."""
    r = compare_rows(amber, width=64, spp=65, seed=SEED, bands=((8, 16), (41, 44)), accel=O.ACCEL_LIST)
    assert r["pixels_differing"] == 0 and r["cast_delta"] == 0 and r["pixels_over_tol"] == 0, r
    assert r["diverged_paths"] == 0 and r["inexact_paths"] == 0 and r["tie_paths"] == 0 and r["signature_kernel_mismatches"] == 0, r

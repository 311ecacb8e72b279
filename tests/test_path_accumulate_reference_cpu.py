"""tests/path_accumulate_reference.py by itself (no GPU): the vectorised restatement of the accumulation contract equals the naive per-pixel loop, and
the inputs of tests/test_path_accumulate.py discriminate -- an accumulator that sums in another order or grouping gives other bits on them."""
import numpy as np
import pytest

import path_accumulate_reference as R


def records_of(n_pixels, n_samples, q, rgb):
    keep = q != R.MARKER
    return q[keep], rgb[keep]


def test_vectorised_equals_the_naive_loop():
    rng = np.random.default_rng(5)
    for n_pixels, n_samples, density in ((1, 1, 1.0), (1, 8, 1.0), (1, 9, 1.0), (3, 31, 1.0), (7, 32, 0.5), (5, 33, 0.3), (3, 64, 1.0), (4, 70, 0.1)):
        q, rgb = R.make_case(n_pixels, n_samples, density, seed=n_pixels * 100 + n_samples)
        fb0 = np.zeros((n_pixels, 3), np.float32)
        a, b = R.accumulate(fb0, n_pixels, n_samples, q, rgb), R.accumulate_naive(fb0, n_pixels, n_samples, q, rgb)
        assert np.array_equal(R.bits(a), R.bits(b)), (n_pixels, n_samples)
        fb1 = np.abs(R.values(rng, n_pixels))                    # a framebuffer that holds something (and no -0)
        a, b = R.accumulate(fb1, n_pixels, n_samples, q, rgb), R.accumulate_naive(fb1, n_pixels, n_samples, q, rgb)
        assert np.array_equal(R.bits(a), R.bits(b)), (n_pixels, n_samples)
        assert np.array_equal(R.bits(R.accumulate(a, n_pixels, n_samples, q, rgb)), R.bits(R.accumulate_naive(a, n_pixels, n_samples, q, rgb)))


def test_special_values_follow_ieee():
    nan, inf, big = np.float32(np.nan), np.float32(np.inf), np.float32(np.finfo(np.float32).max)
    q = np.array([0, 1, 8, R.MARKER, 32, 33, 40, 41, 65], np.uint32)
    rgb = np.array([[-0.0, big, inf], [-0.0, big, -inf], [-0.0, -big, 1.0], [9, 9, 9], [1e-45, nan, 1.0], [-1e-45, 1.0, 1.0], [-0.0, -0.0, -0.0],
                    [1e-40, 2e-40, -3e-40], [0.0, 0.0, 0.0]], np.float32)
    out = R.accumulate(np.zeros((3, 3), np.float32), 3, 32, q, rgb)
    naive = R.accumulate_naive(np.zeros((3, 3), np.float32), 3, 32, q, rgb)
    assert R.same(out, naive).all()
    assert R.bits(out[0, 0]) == 0                                # -0 records onto +0: +0
    assert np.isinf(out[0, 1]) and out[0, 1] > 0                 # big + big overflows within the chunk; the next chunk's -big does not bring it back
    assert np.isnan(out[0, 2])                                   # inf + -inf
    assert R.bits(out[1, 0]) == R.bits(np.float32(1e-40))        # a cancelling pair of subnormals leaves +0; the next chunk's subnormal survives
    assert np.isnan(out[1, 1]) and out[1, 2] == np.float32(2.0)
    assert np.array_equal(R.bits(out[2]), R.bits(np.zeros(3, np.float32)))           # the marker's item and a +0 record leave pixel 2 at +0
    assert not R.same([np.nan, 1.0], [1.0, 1.0]).all() and R.same([np.nan, -0.0], [np.nan, -0.0]).all() and not R.same([0.0], [-0.0]).all()


def test_the_precondition_is_checked():
    with pytest.raises(AssertionError, match="no -0"):
        R.accumulate(np.float32([[-0.0, 0, 0]]), 1, 1, [0], [[1, 1, 1]])


def test_interleave_covers_the_emit_counts():
    rng = np.random.default_rng(3)
    q = np.arange(5000, dtype=np.uint32)
    out_q, out_rgb, counts = R.interleave(rng, q, R.values(rng, 5000))
    assert len(out_q) % 64 == 0 and np.array_equal(out_q[out_q != R.MARKER], q)
    per_trip = (out_q.reshape(-1, 64) != R.MARKER).sum(axis=1)
    assert np.array_equal(per_trip, counts) and {0, 1, 63, 64} <= set(per_trip.tolist()) and len(set(per_trip.tolist())) > 20
    assert (out_rgb[out_q == R.MARKER] == np.float32(1e30)).all()
    out_q, _, counts = R.interleave(rng, q[:0], np.zeros((0, 3), np.float32))
    assert len(out_q) == 64 and (out_q == R.MARKER).all()


def wrong_accumulators(n_pixels, n_samples, m):
    """name -> what an accumulator with one mistake gives on the measurements m, from a cleared framebuffer."""
    fb0 = np.zeros((n_pixels, 3), np.float32)
    rotated = m.copy()
    for p in range(n_pixels):                                   # each pixel's records moved on by one place among its lit samples
        lit = np.flatnonzero((R.bits(m[p]) != 0).any(axis=1))
        if len(lit) > 1:
            rotated[p, lit] = m[p, np.roll(lit, -1)]
    return {
        "sequential": R.accumulate_dense(fb0, m, chunk=n_samples),
        "chunks of 16": R.accumulate_dense(fb0, m, chunk=16),
        "reversed": R.accumulate_dense(fb0, m[:, ::-1, :]),
        "rotated": R.accumulate_dense(fb0, rotated),
    }


@pytest.mark.parametrize("name", list(R.DENSE_CASES))
def test_the_inputs_discriminate(name):
    """On every dense case each wrong accumulator differs from the contract on at least half of the pixels that hold 3 or more records spread over
    2 or more chunks.  A condition on the inputs: if one misses it, the input changes, not the bound."""
    n_pixels, n_samples, density = R.DENSE_CASES[name]
    q, rgb = R.make_case(n_pixels, n_samples, density, R.case_seed(name))
    m = R.dense(n_pixels, n_samples, q, rgb)
    lit = (R.bits(m) != 0).any(axis=2)                           # (n_pixels, n_samples)
    pad = (-n_samples) % R.ACCUM_CHUNK
    chunks = np.pad(lit, ((0, 0), (0, pad))).reshape(n_pixels, -1, R.ACCUM_CHUNK).any(axis=2).sum(axis=1)
    judged = (lit.sum(axis=1) >= 3) & (chunks >= 2)
    right = R.accumulate_dense(np.zeros((n_pixels, 3), np.float32), m)
    if not judged.any():
        assert n_samples <= R.ACCUM_CHUNK                         # the single-chunk cases: nothing to tell apart
        return
    for wrong, out in wrong_accumulators(n_pixels, n_samples, m).items():
        differs = ~R.same(out, right).reshape(n_pixels, 3).all(axis=1)
        share = differs[judged].mean()
        print(f"{name}: {wrong}: differs on {share:.3f} of {int(judged.sum())} pixels")
        if n_samples == R.ACCUM_CHUNK + 1 and wrong in ("sequential", "chunks of 16"):
            # 9 samples from a cleared buffer: the second chunk is one term, (+0 + s) + (+0 + m8) = s + m8 -- the contract IS the sequential sum, whatever
            # the values; no input can tell them apart, so this pair is stated as the identity it is ("reversed" and "rotated" still have to differ)
            assert share == 0.0
            continue
        assert share >= 0.5, (name, wrong, share)

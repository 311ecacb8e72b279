"""tests/denoise_variance_reference.py, the numpy restatement of amber_hip_pt_render_batch's moment update and of amber_hip_pt_denoise_variance's
contract, pinned on its own (no GPU): the GPU tests compare the device's bits with it, so its steps are held here to cases small enough to write out
by hand in scalar binary32 arithmetic, and to the property the filter exists for.

The motivating frame: 48 x 32, flat truth 0.5 in every channel, uniform guides, four batches of one sample; a sample is 16 with probability 1 / 32
and 0 otherwise (default_rng(1)), so a 4-spp mean is 0 in most pixels and 4, 8 or 12 in a few: "a few very bright pixels in black".  All values
are small integers times powers of two, so amber_hip_pt_denoise's sums are exact and "returns its input" can be asserted bit for bit."""
import numpy as np

import denoise_reference as R
import denoise_variance_reference as V

F32 = np.float32
f = F32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def uniform_aov(rows, width, albedo=0.5):
    aov = np.zeros((rows, width, 8), F32)
    aov[..., 0:3], aov[..., 3], aov[..., 6], aov[..., 7] = F32(albedo) * 4, 8, 4, 4      # 4 samples: albedo, depth 2, normal (0, 0, 1)
    return aov


def test_the_moment_update():
    m = np.zeros((1, 2, 4), F32)
    m[0, 1] = (1, 2, 3, 0)
    batch = np.array([[[4, 8, 12], [0, 0, 0]]], F32)
    out = V.moments_update(m, batch, 4)
    y = (f(0.2126) * f(1) + f(0.7152) * f(2)) + f(0.0722) * f(3)
    assert out.dtype == F32 and np.array_equal(bits(out[0, 0]), bits([y, y * y, 1, 0]))
    assert np.array_equal(bits(out[0, 1]), bits([1, 2, 4, 0]))                         # a batch without light still counts
    assert np.array_equal(m[0, 0], np.zeros(4, F32))                                   # the input is left alone
    twice = V.moments_update(out, batch, 4)
    assert np.array_equal(bits(twice[0, 0]), bits([y + y, y * y + y * y, 2, 0]))


def test_a_band_of_one_pixel_returns_its_input_and_var_0():
    fb, aov, m = np.array([[[2, 1, 6]]], F32), uniform_aov(1, 1), np.array([[[3, 5, 2, 0]]], F32)
    # u1 = 1.5, u2 = 2.5, G = 1: v = 2.5 - 2.25 = 0.25, var_0 = 0.25 / 2
    for radius in (0, 1, 3):
        for levels in (1, 5, 8):
            c, var = V.denoise_variance(fb, aov, m, 4, levels=levels, var_radius=radius, with_var=True)
            assert c.shape == (1, 1, 3) and np.array_equal(bits(c), bits([[[0.5, 0.25, 1.5]]])), (radius, levels)
            assert var.shape == (1, 1) and np.array_equal(bits(var), bits([[0.125]])), (radius, levels)
    never = V.denoise_variance(fb, aov, np.zeros((1, 1, 4), F32), 4, with_var=True)
    assert np.array_equal(bits(never[0]), bits([[[0.5, 0.25, 1.5]]])) and np.array_equal(bits(never[1]), bits([[0.0]]))


def test_the_variance_step_by_hand():
    """1 x 3: batches 2 / 0 / 4; pixel 0: u1 = 1, u2 = 2; pixel 2: u1 = 0.5, u2 = 0.75 (all dyadic: every operation is exact)"""
    m = np.array([[[2, 4, 2, 0], [0, 0, 0, 0], [2, 3, 4, 0]]], F32)
    a, n, z, rz = R.guide(uniform_aov(1, 3))
    k = (f(4), f(100), f(10))
    # R = 0: the pixel's own batch variance over its batches; no batches: 0
    assert np.array_equal(bits(V.variance0(m, a, n, z, rz, *k, 0)), bits([[(2 - 1) / 2, 0, (0.75 - 0.25) / 4]]))
    # R = 1, uniform guides (every stop 1): pixel 0 pools itself and pixel 1 (e = 0): unchanged.  Pixel 1 pools both neighbours: A1 = 1.5, A2 = 2.75,
    # G = 2 (its own g = e = 0): mu = 0.75, v = 1.375 - 0.5625 = 0.8125, not divided (batches = 0).  Pixel 2: unchanged.
    assert np.array_equal(bits(V.variance0(m, a, n, z, rz, *k, 1)), bits([[0.5, 0.8125, 0.125]]))
    # an albedo edge between pixels 1 and 2 (0.5 against 0.2: sq * 100 = 27 > 1): pixel 1 pools pixel 0 alone, v = 2 - 1
    aov = uniform_aov(1, 3)
    aov[0, 2, 0:3] = F32(0.2) * 4
    a, n, z, rz = R.guide(aov)
    assert np.array_equal(bits(V.variance0(m, a, n, z, rz, *k, 1)), bits([[0.5, 1.0, 0.125]]))
    assert np.array_equal(bits(V.variance0(m, a, n, z, rz, *k, 3)), bits([[0.5, 1.0, 0.125]]))     # a wider window finds nothing more in 1 x 3
    # all guide constants 0: the edge is open again
    assert np.array_equal(bits(V.variance0(m, a, n, z, rz, f(0), f(0), f(0), 1)), bits([[0.5, 0.8125, 0.125]]))


def test_one_level_by_hand():
    """1 x 2, uniform guides, step 1: pixel 0 has the centre tap and then the tap (dx = 1), pixel 1 the tap (dx = -1) and then the centre; the
    rows above and below are outside.  Scalar binary32 arithmetic, written out."""
    c = np.array([[[1.0, 0.5, 0.25], [1.5, 0.75, 0.5]]], F32)
    var = np.array([[0.5, 0.125]], F32)
    a, n, z, rz = R.guide(uniform_aov(1, 2))
    k_lum = f(16)
    got_c, got_var = V.level(c, var, a, n, z, rz, f(4), f(100), f(10), k_lum, 1)

    def lum(p):
        return (f(0.2126) * p[0] + f(0.7152) * p[1]) + f(0.0722) * p[2]
    l0, l1 = lum(c[0, 0]), lum(c[0, 1])
    w1, w2, w4 = f(1 / 16), f(2 / 16), f(4 / 16)
    v0, v1 = var[0]
    # gv: three rows (all clamped to row 0) of columns (x-1, x, x+1) clamped, row-major, from 0
    gv0 = f(0)
    for row in ((w1, w2, w1), (w2, w4, w2), (w1, w2, w1)):
        for wt, v in zip(row, (v0, v0, v1)):
            gv0 = gv0 + wt * v
    gv1 = f(0)
    for row in ((w1, w2, w1), (w2, w4, w2), (w1, w2, w1)):
        for wt, v in zip(row, (v0, v1, v1)):
            gv1 = gv1 + wt * v
    assert gv0 == f(0.75 * 0.5 + 0.25 * 0.125) and gv1 == f(0.25 * 0.5 + 0.75 * 0.125)
    hc, ht = f(9 / 64), f(3 / 32)                                                    # H[2] * H[2], H[2] * H[1] = H[2] * H[3]
    want_c, want_var = np.zeros((1, 2, 3), F32), np.zeros((1, 2), F32)
    for p, q, lp, lq, gv, centre_first in ((0, 1, l0, l1, gv0, True), (1, 0, l1, l0, gv1, False)):
        r = f(1) / (k_lum * gv + f(1e-10))
        d = lp - lq
        tl = f(1) - (d * d) * r
        assert tl > 0
        e = ((f(1) * f(1)) * f(1)) * tl
        w = ht * (e * e)
        taps = [(hc, p), (w, q)] if centre_first else [(w, q), (hc, p)]
        S, Sv, Sw = np.zeros(3, F32), f(0), f(0)
        for wt, at in taps:
            S = S + wt * c[0, at]
            Sv = Sv + (wt * wt) * var[0, at]
            Sw = Sw + wt
        want_c[0, p], want_var[0, p] = S / Sw, Sv / (Sw * Sw)
    assert np.array_equal(bits(got_c), bits(want_c)) and np.array_equal(bits(got_var), bits(want_var))
    assert (got_var < var.max()).all()                                                 # no per-level scaling: the variance shrinks by itself
    # k_lum = 0 (a cut-off at zero standard deviations: r = 1e10) closes the stop: every pixel keeps its colour and its variance
    shut_c, shut_var = V.level(c, var, a, n, z, rz, f(4), f(100), f(10), f(0), 1)
    assert np.array_equal(bits(shut_c), bits(c)) and np.array_equal(bits(shut_var), bits(var))


def noisy_frame(rows, width, seed):
    rng = np.random.default_rng(seed)
    fb = (rng.random((rows, width, 3)) * 4).astype(F32)
    m = np.zeros((rows, width, 4), F32)
    for _ in range(4):
        m = V.moments_update(m, (rng.random((rows, width, 3))).astype(F32), 1)
    return fb, uniform_aov(rows, width), m


def test_a_pixel_without_batches_and_a_nan_pixel_stay_local():
    rows, width = 21, 23
    fb, aov, m = noisy_frame(rows, width, 3)
    clean = V.denoise_variance(fb, aov, m, 4, levels=2)
    assert np.isfinite(clean).all()
    # NaN colour: 0 * NaN is NaN, so it reaches every pixel that has it for a tap (level 0: +-2, level 1: +-4 more) and no further
    bad = fb.copy()
    bad[10, 11, 1] = np.nan
    out = V.denoise_variance(bad, aov, m, 4, levels=2)
    nan = np.isnan(out).any(axis=-1)
    window = np.zeros((rows, width), bool)
    window[4:17, 5:18] = True
    assert nan[10, 11] and nan.sum() >= 25 and not (nan & ~window).any()
    assert np.array_equal(bits(out)[~window], bits(clean)[~window])
    # a pixel that no batch has touched: e = 0 keeps its moments out of every pool, var_0 comes from its neighbours, everything stays finite, and
    # after one level only the pixels within 3 (the pool) + 1 (the blur) + 2 (the taps) of it change
    hole = m.copy()
    hole[10, 11] = 0
    one = V.denoise_variance(fb, aov, m, 4, levels=1)
    out = V.denoise_variance(fb, aov, hole, 4, levels=1)
    a, n, z, rz = R.guide(aov)
    v0 = V.variance0(hole, a, n, z, rz, f(4), f(100), f(10), 3)
    assert np.isfinite(out).all() and v0[10, 11] > 0
    assert not np.array_equal(bits(out), bits(one)) and np.array_equal(bits(out)[~window], bits(one)[~window])


def fireflies(rows=48, width=32, seed=1):
    rng = np.random.default_rng(seed)
    fb, m = np.zeros((rows, width, 3), F32), np.zeros((rows, width, 4), F32)
    for _ in range(4):
        batch = np.where(rng.random((rows, width)) < 1 / 32, f(16), f(0)).astype(F32)[..., None] * np.ones(3, F32)
        fb, m = fb + batch, V.moments_update(m, batch, 1)
    return fb, uniform_aov(rows, width), m


def test_sparse_fireflies_over_a_flat_truth():
    """the finding this filter answers: amber_hip_pt_denoise with its defaults returns such a frame bit for bit (its colour stop keeps every bright
    pixel apart from its neighbours); the variance-guided filter with its defaults lowers the error"""
    fb, aov, m = fireflies()
    noisy = fb / f(4)
    truth = np.full(fb.shape, 0.5, F32)
    lit = (noisy[..., 0] > 0).mean()
    assert 0.05 < lit < 0.25 and (m[..., 2] == 4).all()
    assert np.array_equal(bits(R.denoise(fb, aov, 4)), bits(noisy))
    out = V.denoise_variance(fb, aov, m, 4)
    e_in, e_out = rmse(noisy, truth), rmse(out, truth)
    print(f"rmse against the flat truth: 4-spp mean {e_in:.4f}, denoise {e_in:.4f} (the input), denoise_variance {e_out:.4f}: {e_out / e_in:.3f} of the input; "
          f"{lit:.3f} of the pixels lit")
    assert np.isfinite(out).all()
    assert e_out < e_in, f"denoise_variance {e_out:.4f} against the input's {e_in:.4f}: ratio {e_out / e_in:.3f}"

"""tests/denoise_reference.py, the numpy restatement of amber_hip_pt_denoise's contract, pinned on its own (no GPU): what the GPU tests compare the
device's bits with must itself separate at a hard guide edge, lower the error of a noisy image and run on bands smaller than its reach.

The seeded image: 37 x 23, columns 0-18 of colour (0.8, 0.2, 0.1) and the rest (0.1, 0.3, 0.9), default_rng(7) normal noise of sigma 0.3, 4 samples
(the sums are 4 times the noisy image: exact).  Guide: albedo 0.7 left and 0.2 right, depth 2, normal (0, 0, 1), coverage 4.  levels = 5,
k = (4, 100, 10, 0): the albedos are 0.5 apart in every channel, so sq * 100 = 75 and no tap crosses the edge; k_color = 0 leaves the colour stop open."""
import numpy as np

import denoise_reference as R

F32 = np.float32
W, HGT, SPLIT, N = 37, 23, 19, 4
K = dict(levels=5, k_normal=4.0, k_albedo=100.0, k_depth=10.0, k_color=0.0)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def seeded():
    clean = np.empty((HGT, W, 3), F32)
    clean[:, :SPLIT] = (0.8, 0.2, 0.1)
    clean[:, SPLIT:] = (0.1, 0.3, 0.9)
    noisy = (clean + np.random.default_rng(7).normal(0.0, 0.3, clean.shape)).astype(F32)
    aov = np.zeros((HGT, W, 8), F32)
    aov[:, :SPLIT, 0:3] = F32(0.7) * F32(N)
    aov[:, SPLIT:, 0:3] = F32(0.2) * F32(N)
    aov[..., 3], aov[..., 6], aov[..., 7] = 2 * N, N, N
    return clean, noisy * F32(N), aov


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def test_the_guide_and_a_constant_image():
    _, fb, aov = seeded()
    a, n, z, rz = R.guide(aov)
    assert np.array_equal(bits(z), bits(np.full((HGT, W), 2, F32))) and np.array_equal(bits(rz), bits(np.full((HGT, W), 0.5, F32)))
    assert np.array_equal(bits(a[:, :SPLIT]), bits(np.full((HGT, SPLIT, 3), 0.7, F32))) and np.array_equal(n[..., 2], np.ones((HGT, W), F32))
    flat = R.denoise(np.full((5, 7, 3), 2.0, F32), np.zeros((5, 7, 8), F32), 4, **K)
    assert np.array_equal(flat, np.full((5, 7, 3), 0.5, F32))                          # a constant image stays what it is: the weights cancel exactly here


def test_a_hard_guide_edge_separates_the_two_sides():
    _, fb, aov = seeded()
    whole = R.denoise(fb, aov, N, **K)
    left = R.denoise(fb[:, :SPLIT], aov[:, :SPLIT], N, **K)
    right = R.denoise(fb[:, SPLIT:], aov[:, SPLIT:], N, **K)
    assert whole.dtype == F32 and whole.shape == (HGT, W, 3)
    assert np.array_equal(bits(whole[:, :SPLIT]), bits(left)) and np.array_equal(bits(whole[:, SPLIT:]), bits(right))


def test_the_error_against_the_clean_image_falls():
    clean, fb, aov = seeded()
    noisy = fb / F32(N)
    guided, unguided = R.denoise(fb, aov, N, **K), R.denoise(fb, np.zeros_like(aov), N, **K)
    e_in, e_guided, e_unguided = rmse(noisy, clean), rmse(guided, clean), rmse(unguided, clean)
    print(f"rmse: input {e_in:.4f}, guided {e_guided:.4f} ({e_guided / e_in:.3f} of the input), all-zero guides {e_unguided:.4f} "
          f"(guided / unguided {e_guided / e_unguided:.3f})")
    assert e_guided < 0.25 * e_in
    assert e_guided < e_unguided


def test_small_shapes():
    _, fb, aov = seeded()
    one = R.denoise(fb[:1, :1], aov[:1, :1], N, **K)
    # a pin of this pixel, not an identity: (c * 9/64) / (9/64) rounds twice
    assert one.shape == (1, 1, 3) and np.array_equal(bits(one), bits(fb[:1, :1] / F32(N)))
    for rows, width in ((1, 40), (9, 5), (3, 33)):                                       # smaller than the level-4 reach of 32 pixels either way
        out = R.denoise(fb[:rows, :width] if width <= W else np.tile(fb[:rows], (1, 2, 1))[:, :width],
                        aov[:rows, :width] if width <= W else np.tile(aov[:rows], (1, 2, 1))[:, :width], N, **K)
        assert out.shape == (rows, width, 3) and np.isfinite(out).all()

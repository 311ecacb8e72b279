"""amber_hip_pt_denoise restated in numpy (a helper, not a test): the contract of include/amber_hip.h operation by operation, every array float32
so that every operation is binary32 and rounded alone.  A tap is a pair of shifted slices: P the pixels whose tap lies inside the band, Q the
taps; pixels outside P get nothing added for that tap.  IEEE division in numpy is correctly rounded, as the device's is."""
import numpy as np

F32 = np.float32
H = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], F32)
DEFAULTS = dict(levels=5, k_normal=4.0, k_albedo=100.0, k_depth=10.0, k_color=0.25)


def sq(u, v):
    d = u - v
    d = d * d
    return (d[..., 0] + d[..., 1]) + d[..., 2]


def clamp0(t):
    return np.where(t > 0, t, F32(0))                                          # a NaN t gives 0


def guide(aov):
    """(a, n, z, rz) of the AOV sums, shape (rows, width, 8) in AmberAovPixel's order"""
    aov = np.ascontiguousarray(aov, F32)
    cov = aov[..., 7]
    hit = cov > 0
    with np.errstate(all="ignore"):
        mean = np.where(hit[..., None], aov[..., :7] / cov[..., None], F32(0))
        a, z, n = mean[..., 0:3], mean[..., 3], mean[..., 4:7]
        rz = np.where(z > 0, F32(1) / z, F32(0))
    return a, n, z, rz


def level(c, a, n, z, rz, k_normal, k_albedo, k_depth, kc, s):
    rows, width = c.shape[:2]
    S, Sw = np.zeros((rows, width, 3), F32), np.zeros((rows, width), F32)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            oy, ox = dy * s, dx * s
            y0, y1, x0, x1 = max(0, -oy), min(rows, rows - oy), max(0, -ox), min(width, width - ox)
            if y0 >= y1 or x0 >= x1:
                continue                                                       # no pixel has this tap inside the band
            P, Q = (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
            hw = H[dy + 2] * H[dx + 2]
            if dy == 0 and dx == 0:
                w = np.full((rows, width), hw, F32)
            else:
                tn = clamp0(F32(1) - sq(n[P], n[Q]) * k_normal)
                ta = clamp0(F32(1) - sq(a[P], a[Q]) * k_albedo)
                tz = clamp0(F32(1) - (np.abs(z[P] - z[Q]) * rz[P]) * k_depth)
                tc = clamp0(F32(1) - sq(c[P], c[Q]) * kc)
                e = ((tn * ta) * tz) * tc
                w = hw * (e * e)
            S[P] = S[P] + w[..., None] * c[Q]
            Sw[P] = Sw[P] + w
    out = S / Sw[..., None]
    assert out.dtype == F32 and S.dtype == F32 and Sw.dtype == F32
    return out


def denoise(fb, aov, n_samples, levels=5, k_normal=4.0, k_albedo=100.0, k_depth=10.0, k_color=0.25):
    """c_levels: what amber_hip_pt_denoise writes as AMBER_RESOLVE_MEAN_F32 for the sums fb (rows, width, 3) and the AOV sums aov (rows, width, 8)"""
    with np.errstate(all="ignore"):
        c = np.ascontiguousarray(fb, F32) / F32(n_samples)
        a, n, z, rz = guide(aov)
        kc = F32(k_color)
        for i in range(levels):
            c = level(c, a, n, z, rz, F32(k_normal), F32(k_albedo), F32(k_depth), kc, 1 << i)
            kc = kc * F32(4)
    return c

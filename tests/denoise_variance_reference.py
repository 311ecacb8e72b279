"""amber_hip_pt_render_batch's moment update and amber_hip_pt_denoise_variance restated in numpy (a helper, not a test): the contract of
include/amber_hip.h operation by operation, every array float32 so that every operation is binary32 and rounded alone.  The guide, the three guide
stops' pieces (sq, clamp0), the tap table H and the slicing of a tap (P the pixels whose tap lies inside the band, Q the taps) are
tests/denoise_reference.py's: the two filters share them as the device code does."""
import numpy as np

import denoise_reference as R

F32 = np.float32
H = R.H
DEFAULTS = dict(levels=5, k_normal=4.0, k_albedo=100.0, k_depth=10.0, k_lum=16.0, var_radius=3)
B3 = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], F32) / F32(16)                # {1,2,1} x {1,2,1} / 16: exact


def lum(c):
    return (F32(0.2126) * c[..., 0] + F32(0.7152) * c[..., 1]) + F32(0.0722) * c[..., 2]


def moments_update(moments, batch, n_samples):
    """the moments (rows, width, 4: m1, m2, batches, pad) after a batch whose sums are `batch` (rows, width, 3): what render_batch's fold adds"""
    m = np.array(moments, F32)
    with np.errstate(all="ignore"):
        y = lum(np.ascontiguousarray(batch, F32) / F32(n_samples))
        m[..., 0] = m[..., 0] + y
        m[..., 1] = m[..., 1] + y * y
        m[..., 2] = m[..., 2] + F32(1)
    return m


def tap(rows, width, oy, ox):
    """(P, Q) of the tap at offset (oy, ox), or None when no pixel has it inside the band"""
    y0, y1, x0, x1 = max(0, -oy), min(rows, rows - oy), max(0, -ox), min(width, width - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def guide_stop(a, n, z, rz, P, Q, k_normal, k_albedo, k_depth):
    tn = R.clamp0(F32(1) - R.sq(n[P], n[Q]) * k_normal)
    ta = R.clamp0(F32(1) - R.sq(a[P], a[Q]) * k_albedo)
    tz = R.clamp0(F32(1) - (np.abs(z[P] - z[Q]) * rz[P]) * k_depth)
    return (tn * ta) * tz


def variance0(moments, a, n, z, rz, k_normal, k_albedo, k_depth, radius):
    """steps 2 and 3: var_0, the variance of the mean"""
    with np.errstate(all="ignore"):
        return _variance0(np.ascontiguousarray(moments, F32), a, n, z, rz, k_normal, k_albedo, k_depth, radius)


def _variance0(m, a, n, z, rz, k_normal, k_albedo, k_depth, radius):
    rows, width = m.shape[:2]
    has = m[..., 2] > 0
    u1 = np.where(has, m[..., 0] / m[..., 2], F32(0))
    u2 = np.where(has, m[..., 1] / m[..., 2], F32(0))
    e = np.where(has, F32(1), F32(0))
    A1, A2, G = (np.zeros((rows, width), F32) for _ in range(3))
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            t = tap(rows, width, dy, dx)
            if t is None:
                continue
            P, Q = t
            g = e[P] if dy == 0 and dx == 0 else guide_stop(a, n, z, rz, P, Q, k_normal, k_albedo, k_depth) * e[Q]
            A1[P] = A1[P] + g * u1[Q]
            A2[P] = A2[P] + g * u2[Q]
            G[P] = G[P] + g
    mu = A1 / G
    v = np.where(G > 0, R.clamp0(A2 / G - mu * mu), F32(0))
    out = np.where(has, v / m[..., 2], v)
    assert out.dtype == F32
    return out


def blur3(var):
    """gv: the 3 x 3 binomial blur at unit spacing, coordinates clamped to the band, summed in row-major order"""
    rows, width = var.shape
    gv = np.zeros((rows, width), F32)
    for dy in (-1, 0, 1):
        yy = np.clip(np.arange(rows) + dy, 0, rows - 1)
        for dx in (-1, 0, 1):
            xx = np.clip(np.arange(width) + dx, 0, width - 1)
            gv = gv + B3[dy + 1, dx + 1] * var[yy][:, xx]
    return gv


def level(c, var, a, n, z, rz, k_normal, k_albedo, k_depth, k_lum, s):
    with np.errstate(all="ignore"):
        return _level(c, var, a, n, z, rz, k_normal, k_albedo, k_depth, k_lum, s)


def _level(c, var, a, n, z, rz, k_normal, k_albedo, k_depth, k_lum, s):
    rows, width = c.shape[:2]
    S, Sv, Sw = np.zeros((rows, width, 3), F32), np.zeros((rows, width), F32), np.zeros((rows, width), F32)
    r = F32(1) / (k_lum * blur3(var) + F32(1e-10))
    l = lum(c)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            t = tap(rows, width, dy * s, dx * s)
            if t is None:
                continue
            P, Q = t
            hw = H[dy + 2] * H[dx + 2]
            if dy == 0 and dx == 0:
                w = np.full((rows, width), hw, F32)
            else:
                d = l[P] - l[Q]
                tl = R.clamp0(F32(1) - (d * d) * r[P])
                e = guide_stop(a, n, z, rz, P, Q, k_normal, k_albedo, k_depth) * tl
                w = hw * (e * e)
            S[P] = S[P] + w[..., None] * c[Q]
            Sv[P] = Sv[P] + (w * w) * var[Q]
            Sw[P] = Sw[P] + w
    out, out_var = S / Sw[..., None], Sv / (Sw * Sw)
    assert out.dtype == F32 and out_var.dtype == F32 and r.dtype == F32
    return out, out_var


def denoise_variance(fb, aov, moments, n_samples, levels=5, k_normal=4.0, k_albedo=100.0, k_depth=10.0, k_lum=16.0, var_radius=3, with_var=False):
    """c_levels: what amber_hip_pt_denoise_variance writes as AMBER_RESOLVE_MEAN_F32 for the sums fb (rows, width, 3), the AOV sums aov (rows, width, 8)
    and the moments (rows, width, 4); with_var: (c_levels, var_levels)"""
    k = [F32(k_normal), F32(k_albedo), F32(k_depth)]
    with np.errstate(all="ignore"):
        c = np.ascontiguousarray(fb, F32) / F32(n_samples)
        a, n, z, rz = R.guide(aov)
        var = variance0(moments, a, n, z, rz, *k, var_radius)
        for i in range(levels):
            c, var = level(c, var, a, n, z, rz, *k, F32(k_lum), 1 << i)
    return (c, var) if with_var else c

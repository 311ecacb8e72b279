"""amber_hip_pt_temporal restated in numpy (a helper, not a test): the contract of include/amber_hip.h operation by operation, every array float32 so
that every operation is binary32 and rounded alone.  The guide record, the guide stops and the levels are tests/denoise_reference.py's.  A tap is a
gather with clamped coordinates: a tap that is not taken reads the pixel's own record and adds +0, which is what "nothing is added" means for sums
that start at +0.  IEEE division and square root in numpy are correctly rounded, as the device's are.

    state = empty_state(rows, width)
    out, state, info = temporal(state, fb, aov, n_samples, lens, sensor, row_begin=0, levels=0, ...)

`lens` is a Lens (lens_of(FlatThinLens) or make_lens(...)), `sensor` (W, H, scene_width, scene_height).  `info` says what happened to every pixel:
kept (the history was kept), taps (accepted taps), fractional (kept through two or more accepted taps of non-zero weight)."""
from collections import namedtuple

import numpy as np

import denoise_reference as D

F32 = np.float32
DEFAULTS = dict(levels=5, max_history=32, k_normal=4.0, k_albedo=100.0, k_depth=10.0, k_color=0.25)
Lens = namedtuple("Lens", "origin global_ local_ sensor_distance words")


def lens_of(flat):
    """the values of an AmberFlatThinLens (amber_amd.api.FlatThinLens) the call uses, and the words an unchanged lens is recognised by"""
    f = lambda a: np.array(list(a), F32)
    words = (f(flat.origin).tobytes() + f(flat.global_).tobytes() + f(flat.local_).tobytes() +
             np.array([flat.focus_distance, flat.sensor_distance, flat.p_area], F32).tobytes() + np.array([flat.n_blades, flat.kind], np.uint32).tobytes())
    return Lens(f(flat.origin), f(flat.global_), f(flat.local_), F32(flat.sensor_distance), words)


def make_lens(origin, global_, sensor_distance):
    """a lens from a world position, a 3 x 3 matrix lens-local -> world (row-major) and a sensor distance; local_ is the inverse, narrowed to binary32"""
    g = np.asarray(global_, np.float64).reshape(3, 3)
    o, g32, l32 = np.array(origin, F32), g.astype(F32).reshape(9), np.linalg.inv(g).astype(F32).reshape(9)
    return Lens(o, g32, l32, F32(sensor_distance), o.tobytes() + g32.tobytes() + l32.tobytes() + F32(sensor_distance).tobytes())


def lum(c):
    return (F32(0.2126) * c[..., 0] + F32(0.7152) * c[..., 1]) + F32(0.0722) * c[..., 2]


def matvec(m, v):
    return [(m[3 * r] * v[0] + m[3 * r + 1] * v[1]) + m[3 * r + 2] * v[2] for r in range(3)]


def dot(v):
    return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]


def empty_state(rows, width):
    z = lambda *s: np.zeros((rows, width) + s, F32)
    return dict(hist=z(8), guide=(z(3), z(3), z(), z()), lens=None, empty=True)


def reset(state):
    rows, width = state["hist"].shape[:2]
    return dict(empty_state(rows, width), guide=state["guide"], lens=state["lens"])


def accumulate(state, fb, aov, n_samples, lens, sensor, row_begin=0, max_history=32, k_normal=4.0, k_albedo=100.0, k_depth=10.0):
    """steps 1 to 4: (new state, info); new state["hist"] is what amber_hip_pt_history_download returns"""
    fb, aov = np.ascontiguousarray(fb, F32), np.ascontiguousarray(aov, F32)
    rows, width = fb.shape[:2]
    W, Hh, sw, sh = sensor
    wf, hf, sw, sh = F32(W), F32(Hh), F32(sw), F32(sh)
    k_normal, k_albedo, k_depth, cap = F32(k_normal), F32(k_albedo), F32(k_depth), F32(max_history)
    with np.errstate(all="ignore"):
        c = fb / F32(n_samples)
        a, n, z, rz = D.guide(aov)
        covered = aov[..., 7] > 0
        Y = lum(c)
        ly, px = np.mgrid[0:rows, 0:width]
        H1, (a1, n1, z1, rz1) = state["hist"], state["guide"]
        empty = state["empty"]
        moved = not empty and state["lens"].words != lens.words
        usable = np.full((rows, width), not empty)
        ix, iy = px.astype(np.int64), ly.astype(np.int64)                         # iy: local rows
        one, zero = np.ones((rows, width), F32), np.zeros((rows, width), F32)
        b, d = [one, zero, zero, zero], z
        if moved:
            before = state["lens"]
            uvx, uvy = (px.astype(F32) + F32(0.5)) / wf, ((ly + row_begin).astype(F32) + F32(0.5)) / hf
            s = [(uvx - F32(0.5)) * sw, (uvy - F32(0.5)) * sh, np.full((rows, width), lens.sensor_distance, F32)]
            g = matvec(lens.global_, [-s[0], -s[1], -s[2]])
            length = np.sqrt(dot(g))
            P = [lens.origin[i] + z * (g[i] / length) for i in range(3)]
            v = [P[i] - before.origin[i] for i in range(3)]
            dl = matvec(before.local_, v)
            t = before.sensor_distance / dl[2]
            fx, fy = (t * dl[0] / sw + F32(0.5)) * wf - F32(0.5), (t * dl[1] / sh + F32(0.5)) * hf - F32(0.5)
            d = np.sqrt(dot(v))
            valid = (dl[2] < 0) & (fx > -1) & (fx < wf) & (fy > -1) & (fy < hf)
            usable = usable & valid & covered
            flx, fly = np.where(valid, np.floor(fx), F32(0)), np.where(valid, np.floor(fy), F32(0))
            ax, ay = fx - flx, fy - fly
            ux, uy = F32(1) - ax, F32(1) - ay
            b = [ux * uy, ax * uy, ux * ay, ax * ay]
            ix, iy = flx.astype(np.int64), fly.astype(np.int64) - row_begin
        rd = F32(1) / d
        S, B = np.zeros((rows, width, 6), F32), np.zeros((rows, width), F32)
        taps, weighted = np.zeros((rows, width), np.int64), np.zeros((rows, width), np.int64)
        for k in range(4):
            qx, qy = ix + (k & 1), iy + (k >> 1)
            inside = (qx >= 0) & (qx < width) & (qy >= 0) & (qy < rows) & (k == 0 or moved)
            qx, qy = np.where(inside, qx, px), np.where(inside, qy, ly)
            Hq = H1[qy, qx]
            had = rz1[qy, qx] > 0
            tn = D.clamp0(F32(1) - D.sq(n, n1[qy, qx]) * k_normal)
            ta = D.clamp0(F32(1) - D.sq(a, a1[qy, qx]) * k_albedo)
            tz = D.clamp0(F32(1) - (np.abs(d - z1[qy, qx]) * rd) * k_depth)
            stop = (tn * ta) * tz
            take = usable & inside & (Hq[..., 3] > 0) & np.where(covered, had & (stop > 0), ~had)
            S = S + np.where(take[..., None], b[k][..., None] * Hq[..., :6], F32(0))
            B = B + np.where(take, b[k], F32(0))
            taps += take
            weighted += take & (b[k] > 0)
        kept = B > F32(0.01)
        h = S / B[..., None]
        grown = h[..., 3] + F32(1)
        N = np.where(grown < cap, grown, cap)
        alpha = F32(1) / N
        now = np.stack([c[..., 0], c[..., 1], c[..., 2], Y, Y * Y], axis=-1)
        old = h[..., [0, 1, 2, 4, 5]]
        blend = old + (now - old) * alpha[..., None]
        new = np.where(kept[..., None], blend, now)
        hist = np.zeros((rows, width, 8), F32)
        hist[..., 0:3], hist[..., 3], hist[..., 4:6] = new[..., 0:3], np.where(kept, N, F32(1)), new[..., 3:5]
    assert hist.dtype == F32 and S.dtype == F32 and B.dtype == F32 and h.dtype == F32 and blend.dtype == F32 and d.dtype == F32
    info = dict(kept=kept, taps=taps, fractional=kept & (weighted >= 2), moved=moved)
    return dict(hist=hist, guide=(a, n, z, rz), lens=lens, empty=False), info


def temporal(state, fb, aov, n_samples, lens, sensor, row_begin=0, levels=5, max_history=32, k_normal=4.0, k_albedo=100.0, k_depth=10.0, k_color=0.25):
    """(what amber_hip_pt_temporal writes as AMBER_RESOLVE_MEAN_F32, new state, info)"""
    state, info = accumulate(state, fb, aov, n_samples, lens, sensor, row_begin, max_history, k_normal, k_albedo, k_depth)
    c = state["hist"][..., 0:3].copy()
    a, n, z, rz = state["guide"]
    with np.errstate(all="ignore"):
        kc = F32(k_color)
        for i in range(levels):
            c = D.level(c, a, n, z, rz, F32(k_normal), F32(k_albedo), F32(k_depth), kc, 1 << i)
            kc = kc * F32(4)
    return c, state, info

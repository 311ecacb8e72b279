"""amber_hip_lt_trace_photons restated: the vertices of the light paths, from the oracle's exported stages only.

The walker has no code of its own for the physics.  Light path i of pass s starts its sampler at oracle_xorshift_seed(seed + 0x6C74, i, s), takes its
first ray from oracle_light_rays, and then repeats the loop of algorithm_lt.cc:135-162: oracle_cast; a vertex record where the cast hits (before the
material is sampled); oracle_sample_material_xorshift with importance = 1, the state advanced by the count it returns; the roulette draw
(f64_reference.xorshift_uniform) against p = min(0.9375, max(w)); weight = weight * (w / p).  Every operation on floats is a binary32 numpy operation.

test_photon_reference_cpu.py pins it to the pinned oracle: its Eye vertices, put through oracle_lens_responses and weight * value / (W * H), are the
records of oracle_render_lt_xorshift bit for bit, and its casts are the oracle's.
"""
import ctypes as C

import numpy as np

import f64_reference
import oracle_binding as O
from test_lt_render_pass import LIGHTS

# amber_amd.api.PHOTON_DTYPE, restated (this module runs without the package)
PHOTON = np.dtype([("pos", np.float32, (3,)), ("object", np.int32), ("dir_out", np.float32, (3,)), ("path", np.uint32),
                   ("weight", np.float32, (3,)), ("sample", np.uint32), ("normal", np.float32, (3,)), ("bounce", np.uint32)])
DIFFUSE, SPECULAR, LIGHT, EYE, ALL = 1, 2, 4, 8, 15
MASK_OF_KIND = np.array([DIFFUSE, DIFFUSE, SPECULAR, SPECULAR, LIGHT, EYE], np.uint32)      # Lambertian, Phong, Specular, Refraction, DiffuseLight, Eye

# The scene of the tests: test_lt_render_pass's lights scene plus a Phong sphere in front of the glass sphere -- all six material kinds, all four primitive kinds
SCENE = dict(LIGHTS)
SCENE["materials"] = LIGHTS["materials"] + [(1, (0.6, 0.5, 0.4), 20.0)]
SCENE["objects"] = LIGHTS["objects"][:-1] + [(1, 5, [-0.9, -0.6, -0.6, 0.4])] + LIGHTS["objects"][-1:]
W, H, SEED, SCALE, PASSES = 24, 16, 13, 16, 16


def oracle_sensor(width, height, scale):
    return O.OSensor(width, height, np.float32(0.036 * scale), np.float32(0.036 / width * height * scale))


def oracle_scene(accel=O.ACCEL_LIST, scene=None):
    return O.Scene.create(accel=accel, **(SCENE if scene is None else scene))


class Walker:
    def __init__(self, osc, seed, max_depth=0):
        self.osc, self.seed, self.max_depth = osc, seed, max_depth
        self.L = O.load()
        self.mats = []
        for kind, rho, param, _ in osc.materials():
            self.mats.append(O.OMaterial(int(kind), (C.c_float * 3)(*[float(x) for x in rho]), float(param)))
        self.mat_of = [int(o[1]) for o in osc.objects()]
        self.casts = 0

    def path(self, i, s, out):
        """Appends the vertices of light path i of pass s to `out` (tuples in PHOTON's field order); counts the casts."""
        L = self.L
        state0 = L.oracle_xorshift_seed(self.seed + 0x6C74, i, s)
        o, d, weight, _, after = self.osc.light_rays(np.array([state0], np.uint64))
        o, d, weight = o[0].copy(), d[0].copy(), weight[0].copy()
        state = after.copy()                                                   # uint64 array of one: xorshift_uniform updates it in place
        k = 0
        while True:
            idx, _, pos, nrm = self.osc.cast(o, d)
            k += 1
            self.casts += 1
            if idx < 0:
                return
            m = self.mats[self.mat_of[idx]]
            dir_out = -d
            out.append((pos, idx, dir_out, i, weight.copy(), s, nrm, k))
            dir_in, sw = np.zeros(3, np.float32), np.zeros(3, np.float32)
            n, do = np.ascontiguousarray(nrm, np.float32), np.ascontiguousarray(dir_out, np.float32)
            used = L.oracle_sample_material_xorshift(C.byref(m), n.ctypes.data, do.ctypes.data, int(state[0]), 1, O._m(None), dir_in.ctypes.data, sw.ctypes.data)
            for _ in range(used):
                f64_reference.xorshift_uniform(state)
            p = np.float32(0.9375)
            if sw.max() < p:
                p = sw.max()
            if f64_reference.xorshift_uniform(state)[0] >= p:
                return
            if self.max_depth and k >= self.max_depth:
                return
            o, d = pos, dir_in
            weight = weight * (sw / p)

    def run(self, first_sample, n_samples, path_begin, path_end):
        """The records of amber_hip_lt_trace_photons(first_sample, n_samples, path_begin, path_end, ALL): (sample, path, bounce) order by construction."""
        rows = []
        for s in range(first_sample, first_sample + n_samples):
            for i in range(path_begin, path_end):
                self.path(i, s, rows)
        rec = np.zeros(len(rows), PHOTON)
        for j, r in enumerate(rows):
            rec[j] = r
        return rec

    def kinds(self, rec):
        """Material kind of every record's object."""
        return np.array([self.mats[self.mat_of[int(o)]].kind for o in rec["object"]], np.uint32)

    def select(self, rec, surfaces):
        """What a call with the mask `surfaces` returns of the ALL list."""
        return rec[(MASK_OF_KIND[self.kinds(rec)] & np.uint32(surfaces)) != 0]


def select_len(walker, rec, surfaces):
    return len(walker.select(rec, surfaces))


def splats_of(walker, rec, width, height, scale):
    """The Eye vertices through the lens: (k, 7) uint32 rows {path, sample, bounce, pixel, rgb bits}, the layout of oracle_render_lt_xorshift's records."""
    eye = rec[walker.kinds(rec) == 5]
    s = oracle_sensor(width, height, scale)
    n = len(eye)
    pos, dout = np.ascontiguousarray(eye["pos"]), np.ascontiguousarray(eye["dir_out"])
    reached, pixel, value = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.float32)
    walker.L.oracle_lens_responses(walker.osc.h, C.byref(s), n, pos.ctypes.data, dout.ctypes.data, O._m(None), reached.ctypes.data, pixel.ctypes.data, value.ctypes.data)
    add = (eye["weight"] * value[:, None]) / np.float32(width * height)
    out = np.zeros((n, 7), np.uint32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = eye["path"], eye["sample"], eye["bounce"], pixel
    out[:, 4:7] = np.ascontiguousarray(add, np.float32).view(np.uint32)
    return out[reached != 0], n


def oracle_splats(osc, width, height, scale, seed, first, n, max_depth=0):
    """oracle_render_lt_xorshift on the enlarged sensor: (records (k, 7) uint32, casts)."""
    s = oracle_sensor(width, height, scale)
    img = np.zeros((height, width, 3), np.float32)
    cnt = O.OCounters()
    rec = np.zeros((1 << 16, 7), np.uint32)
    k = O.load().oracle_render_lt_xorshift(osc.h, C.byref(s), seed, first, n, O._m(None), max_depth, img.ctypes.data, C.byref(cnt), rec.ctypes.data, len(rec))
    assert k <= len(rec)
    return rec[:k], int(cnt.casts)


_cache = {}


def reference(max_depth=0, accel=O.ACCEL_LIST):
    """(walker, records of ALL over the tests' frame and passes), computed once per (max_depth, accel) and left unchanged."""
    key = (max_depth, accel)
    if key not in _cache:
        w = Walker(oracle_scene(accel), SEED, max_depth)
        rec = w.run(0, PASSES, 0, W * H)
        rec.setflags(write=False)
        _cache[key] = (w, rec)
    return _cache[key]

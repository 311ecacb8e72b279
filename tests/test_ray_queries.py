"""amber_hip_pt_cast_rays / amber_hip_pt_occluded on the GPU (amber_amd/csrc/hip/ray_query.inc): the caller's rays through the handle's engine.

Every ray of every case is compared with the oracle, bit for bit on object and t: oracle_cast_many(ACCEL_LIST) for engines LIST, TWO_PHASE, BVH and
AUTO, ACCEL_BVH for REFERENCE_BVH; pos and normal against oracle_cast on 4096 hits per scene; occluded against `oracle t <= t_max` in numpy.  The
oracle's answer does not depend on t_max, so it is computed once per scene on the base rays and every base ray is then queried under seven t_max
values: INFINITY, 0, a negative number, NaN, exactly its own hit distance (must be reported), the next binary32 number below it (must be a miss:
the filter rule), a random fraction of the scene diagonal.

Batch edges (the last section): counts below, at and just above a wave and a block of 256 with every ray compared and the output arrays guarded
by sentinels; AMBER_RAYS_HOST calls of one, two and three trips through the staging buffers (2^20 rays a trip) in both orders of occluded and
cast on one handle; the same counts through the device-pointer path in the torch child.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle_binding as O
import scene_files as SF
from amber_amd import scenes
from bvh_parity import bits
from fuzz_scenes import scene_for_seed
from test_device_build import _objects

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
N_VARIANTS = 7


# ---- rays ------------------------------------------------------------------------------------------------------------------------------
def scene_box(arr):
    """(lo, hi, diagonal) of the objects' anchor points (centre / first vertex), widened by half a unit as the random rays of the other tests are"""
    c = arr["p"][:, :3]
    lo, hi = np.nanmin(c, 0) - 0.5, np.nanmax(c, 0) + 0.5
    return lo, hi, float(np.linalg.norm(hi - lo))


def base_rays(osc, arr, frame, seed):
    """The engine's own path rays of a few rows + the stress sets of the issue.  Returns (origins, dirs) float32."""
    W, H, fseed, rows, spp = frame
    rng = np.random.default_rng(seed)
    lo, hi, diag = scene_box(arr)
    centre = 0.5 * (lo + hi)
    c = arr["p"][:, :3]
    sets = [osc.collect_rays(W, H, fseed, 0, spp, rows, 40_000)]                            # the engine's own eye and secondary rays

    def towards(o, n):
        d = c[rng.integers(0, len(c), n)] + rng.normal(size=(n, 3)) * 0.02 - o
        return d / np.linalg.norm(d, axis=1, keepdims=True)
    n = 40_000                                                                             # uniform origins in the box, |d| from 0.5 to 2
    o = rng.uniform(lo, hi, (n, 3))
    sets.append((o, towards(o, n) * rng.uniform(0.5, 2.0, (n, 1))))
    for far in (10.0, 1e4):                                                                # origins 10 and 1e4 diagonals outside
        n = 8_000
        u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
        o = (centre + u * far * diag).astype(F32).astype(np.float64)
        sets.append((o, towards(o, n)))
    n = 6_000                                                                              # axis-parallel directions through object anchors
    axis = rng.integers(0, 3, n); sign = rng.choice([-1.0, 1.0], n)
    d = np.zeros((n, 3)); d[np.arange(n), axis] = sign
    o = c[rng.integers(0, len(c), n)].astype(np.float64) - d * rng.uniform(0.1, 2.0, (n, 1))
    sets.append((o, d))
    d2 = d.copy()                                                                          # ... and the same with denormal components beside the axis
    d2[np.arange(n), (axis + 1) % 3] = rng.choice([1e-40, -1e-40, 1.4e-45], n)
    d2[np.arange(n), (axis + 2) % 3] = rng.choice([0.0, 3e-39, -1e-42], n)
    sets.append((o, d2))
    n = 64                                                                                 # zero direction (inside a sphere the reference's test still accepts)
    sets.append((c[rng.integers(0, len(c), n)].astype(np.float64) + rng.normal(size=(n, 3)) * 0.01, np.zeros((n, 3))))
    n = 6 * 32                                                                             # NaN in each of the six components
    o = rng.uniform(lo, hi, (n, 3)); d = towards(o, n)
    od = np.concatenate([o, d], 1); od[np.arange(n), np.arange(n) % 6] = np.nan
    sets.append((od[:, :3], od[:, 3:]))
    org = np.ascontiguousarray(np.concatenate([s[0] for s in sets]), F32)
    dirs = np.ascontiguousarray(np.concatenate([s[1] for s in sets]), F32)
    return org, dirs


def with_t_max(org, dirs, t_oracle, diag, seed):
    """every base ray under the seven t_max values: (origins, dirs, t_max, index of the base ray)"""
    rng = np.random.default_rng(seed)
    n = len(org)
    known = np.where(np.isnan(t_oracle), F32(np.inf), t_oracle).astype(F32)
    variants = [np.full(n, np.inf, F32), np.zeros(n, F32), np.full(n, -1.5, F32), np.full(n, np.nan, F32), known,
                np.nextafter(known, F32(-np.inf)), (rng.uniform(0, 1, n) * diag).astype(F32)]
    assert len(variants) == N_VARIANTS
    idx = np.tile(np.arange(n), N_VARIANTS)
    return org[idx], dirs[idx], np.concatenate(variants), idx


def expected(obj_o, t_o, t_max):
    """the filter rule in numpy: reported iff the oracle hit and t <= t_max (NaN compares false)"""
    with np.errstate(invalid="ignore"):
        rep = (obj_o >= 0) & (t_o <= t_max)
    return rep, np.where(rep, obj_o, -1).astype(np.int32), np.where(rep, t_o, F32(np.nan)).astype(F32)


def check_queries(pt, label, q, exp, osc_cast=None, subsample=4096):
    """cast_rays and occluded of one handle against the expectation, every ray; pos / normal against oracle_cast on a subsample of the hits"""
    o, d, tm, _ = q
    rep, obj_e, t_e = exp
    obj, t, pos, nrm = pt.cast_rays(o, d, tm)
    occ = pt.occluded(o, d, tm)
    bad = obj != obj_e
    print(f"\n{label}: {len(o)} rays, {int(rep.sum())} reported hits, object mismatches {int(bad.sum())}, "
          f"t mismatches {int((bits(t) != bits(t_e))[rep].sum())}, occluded mismatches {int((occ != rep).sum())}")
    assert not bad.any(), (label, np.flatnonzero(bad)[:8], obj[bad][:8], obj_e[bad][:8], o[bad][:4], d[bad][:4], tm[bad][:8])
    assert np.array_equal(bits(t)[rep], bits(t_e)[rep]), label
    assert np.isnan(t[~rep]).all() and not pos[~rep].any() and not nrm[~rep].any(), label             # a miss: t = NaN, pos = normal = 0
    assert np.array_equal(occ, rep), (label, np.flatnonzero(occ != rep)[:8])
    if osc_cast is not None:
        hits = np.flatnonzero(rep)
        pick = hits[np.random.default_rng(5).choice(len(hits), min(subsample, len(hits)), replace=False)]
        assert len(pick) >= min(subsample, 4096)
        for i in pick:
            oi, ot, op, on = osc_cast.cast(o[i], d[i])
            assert oi == obj[i] and bits(ot) == bits(t[i]) and np.array_equal(bits(op), bits(pos[i])) and np.array_equal(bits(on), bits(nrm[i])), (label, int(i))
    return obj, t, pos, nrm, occ


class Case:
    """One scene: host scene, oracle scene (created with ACCEL_BVH: serves LIST and the reference's BVH), base rays, the oracle's answers, the queries"""
    def __init__(self, amber, name, hs, osc, frame, seed=3):
        self.amber, self.name, self.hs, self.osc, self.frame = amber, name, hs, osc, frame
        self.arr = _objects(hs)
        self.diag = scene_box(self.arr)[2]
        osc.set_accel(O.ACCEL_LIST)
        self.org, self.dirs = base_rays(osc, self.arr, frame, seed)
        self.oracle = {}
        for accel in (O.ACCEL_LIST, O.ACCEL_BVH):
            self.oracle[accel] = osc.cast_many(self.org, self.dirs, accel, threads=16)
        obj_l, t_l = self.oracle[O.ACCEL_LIST]
        assert (obj_l >= 0).sum() > 20_000, name
        self.q = with_t_max(self.org, self.dirs, t_l, self.diag, seed + 1)
        self.exp = {a: expected(self.oracle[a][0][self.q[3]], self.oracle[a][1][self.q[3]], self.q[2]) for a in self.oracle}
        # exactly the hit distance is reported, the number below it is a miss (variants 4 and 5 of the List expectation)
        n = len(self.org)
        hit = obj_l >= 0
        assert self.exp[O.ACCEL_LIST][0][4 * n:5 * n][hit].all() and not self.exp[O.ACCEL_LIST][0][5 * n:6 * n].any()

    def tracer(self, engine=0, device=False, **kw):
        a = self.amber
        W, H, seed, rows, _ = self.frame
        return a.PathTracer(self.hs, a.Sensor.default(W, H), seed=seed, rows=rows, engine=engine, flags=a.PT_FLAG_DEVICE_BUILD if device else 0, **kw)

    def check(self, engine, label, device=False, pos=False):
        accel = O.ACCEL_BVH if engine == self.amber.ENGINE_REFERENCE_BVH else O.ACCEL_LIST
        pt = self.tracer(engine, device)
        self.osc.set_accel(accel)
        out = check_queries(pt, f"{self.name}, {label}", self.q, self.exp[accel], self.osc if pos else None)
        pt.close()
        return out


FRAME = (256, 256, 12345, (120, 124), 4)
SPHERE_FRAME = (1024, 1024, 7, (500, 502), 2)
_cases = {}


def _case(amber, key):
    """the Case of one of the three scenes several tests share: built, and its rays put through the oracle, once"""
    if key not in _cases:
        if key == "cornell":
            _cases[key] = Case(amber, "Cornell box", amber.HostScene.cornell_box(), O.Scene.cornell(O.ACCEL_BVH), FRAME)
        elif key == "cornell20":
            kw = scenes.cornell_plus(20)
            assert 40 <= len(kw["kinds"]) + kw["n_blades"] <= 60
            _cases[key] = Case(amber, "Cornell + 20", amber.HostScene.create_arrays(**kw), O.Scene.create_arrays(**kw, accel=O.ACCEL_BVH), FRAME)
        else:
            kw = scenes.random_spheres(20_000, 7)
            _cases[key] = Case(amber, "20 000 spheres", amber.HostScene.create_arrays(**kw), O.Scene.create_arrays(**kw, accel=O.ACCEL_BVH), SPHERE_FRAME)
    return _cases[key]


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------------
def test_cornell_box_every_engine(amber):
    """AUTO picks TWO_PHASE (19 objects)"""
    c = _case(amber, "cornell")
    c.check(amber.ENGINE_AUTO, "AUTO (two-phase)", pos=True)
    for engine, label in ((amber.ENGINE_LIST, "LIST"), (amber.ENGINE_TWO_PHASE, "TWO_PHASE"), (amber.ENGINE_BVH, "BVH")):
        c.check(engine, label)
    c.check(amber.ENGINE_REFERENCE_BVH, "REFERENCE_BVH", pos=True)
    if amber.is_lab():
        c.check(amber.ENGINE_WAVEFRONT, "WAVEFRONT (answers as AUTO)")


def test_grouped_two_phase_scene(amber):
    """45 objects: AUTO is the two-phase engine over groups of 32"""
    c = _case(amber, "cornell20")
    assert 40 <= len(c.arr) <= 60
    c.check(amber.ENGINE_AUTO, "AUTO (grouped two-phase)", pos=True)
    for engine, label in ((amber.ENGINE_TWO_PHASE, "TWO_PHASE"), (amber.ENGINE_LIST, "LIST"), (amber.ENGINE_BVH, "BVH"), (amber.ENGINE_REFERENCE_BVH, "REFERENCE_BVH")):
        c.check(engine, label)


def test_sphere_scene_host_and_device_trees(amber):
    c = _case(amber, "spheres")
    host = c.check(amber.ENGINE_AUTO, "AUTO (BVH), host tree", pos=True)
    dev = c.check(amber.ENGINE_AUTO, "AUTO (BVH), device tree", device=True)
    for a, b in zip(host, dev):
        assert a.tobytes() == b.tobytes()
    c.check(amber.ENGINE_LIST, "LIST")
    c.check(amber.ENGINE_REFERENCE_BVH, "REFERENCE_BVH")


def test_fuzz_scene_with_every_primitive_kind(amber):
    kw, _ = scene_for_seed(7)                                                 # seed % 4 == 3: a big scene (40 .. 400 objects)
    assert {k for k, _, _ in kw["objects"]} == {0, 1, 2, 3}
    c = Case(amber, "fuzz scene 7", amber.HostScene.create(**kw), O.Scene.create(**kw, accel=O.ACCEL_BVH), FRAME)
    c.check(amber.ENGINE_AUTO, "AUTO", pos=True)
    for engine, label in ((amber.ENGINE_LIST, "LIST"), (amber.ENGINE_BVH, "BVH host tree"), (amber.ENGINE_REFERENCE_BVH, "REFERENCE_BVH")):
        c.check(engine, label)
    c.check(amber.ENGINE_BVH, "BVH device tree", device=True)


def test_small_triangle_mesh(amber, tmp_path):
    path, objects, materials = SF.write_scene(tmp_path, subdivisions=2)
    osc = O.Scene.create(objects, materials, SF.TRANSFORM, accel=O.ACCEL_BVH | O.BLADES_LAST, **SF.LENS)
    c = Case(amber, "imported mesh", amber.HostScene.import_file(path), osc, FRAME)
    c.check(amber.ENGINE_AUTO, "AUTO (BVH)", pos=True)
    c.check(amber.ENGINE_AUTO, "AUTO (BVH), device tree", device=True)
    c.check(amber.ENGINE_LIST, "LIST")
    c.check(amber.ENGINE_REFERENCE_BVH, "REFERENCE_BVH")


# ---- a live handle ---------------------------------------------------------------------------------------------------------------------------
def test_queries_follow_update_objects(amber):
    """REFIT and REBUILD: queries after the update equal the oracle of the new scene; a query enqueued BEFORE it (device pointers, asynchronous)
    answers for the old scene.  The asynchronous part runs in the torch child below; here: the synchronous order."""
    from test_update_objects import moved
    kw = scenes.random_spheres(20_000, 7)
    kw_b = moved(kw, 101)
    frame = (1024, 1024, 7, (500, 502), 2)
    a = Case(amber, "spheres A", amber.HostScene.create_arrays(**kw), O.Scene.create_arrays(**kw, accel=O.ACCEL_BVH), frame)
    b = Case(amber, "spheres B", amber.HostScene.create_arrays(**kw_b), O.Scene.create_arrays(**kw_b, accel=O.ACCEL_BVH), frame)
    for mode, label, device in ((amber.UPDATE_REFIT, "REFIT", False), (amber.UPDATE_REBUILD, "REBUILD", True)):
        pt = a.tracer(device=device)
        check_queries(pt, f"before {label}", a.q, a.exp[O.ACCEL_LIST])
        info = pt.update_flat(0, b.arr, mode)
        assert info["mode_used"] == mode
        check_queries(pt, f"after {label}: scene B's rays", b.q, b.exp[O.ACCEL_LIST])
        pt.update_flat(0, a.arr, mode)
        check_queries(pt, f"after {label} back to A", a.q, a.exp[O.ACCEL_LIST])
        pt.close()


# ---- side effects and errors -------------------------------------------------------------------------------------------------------------
def test_queries_leave_the_render_alone(amber):
    c = _case(amber, "cornell")
    kw = scenes.random_spheres(20_000, 7)
    for hs in (c.hs, amber.HostScene.create_arrays(**kw)):
        res = []
        for queries in (False, True):
            pt = amber.PathTracer(hs, amber.Sensor.default(128, 128), seed=9, rows=(60, 68))
            pt.render_pass(0, 16)
            before = pt.kernel_time()
            if queries:
                pt.cast_rays(c.org, c.dirs); pt.occluded(c.org, c.dirs, 0.5)
                assert pt.kernel_time() == before                              # no launch counted, no time added
            pt.render_pass(16, 16)
            img, rays = pt.download()
            res.append((bits(img).copy(), rays, pt.kernel_time()[0]))
            pt.close()
        assert res[0][1] == res[1][1] and np.array_equal(res[0][0], res[1][0]) and res[0][2] == res[1][2]


def test_errors_leave_the_handle_as_it_was(amber):
    lib = amber.load_library()
    hs = amber.HostScene.create_arrays(**scenes.random_spheres(5_000, 7))
    for engine in (amber.ENGINE_AUTO, amber.ENGINE_LIST):
        pt = amber.PathTracer(hs, amber.Sensor.default(64, 64), seed=2, engine=engine)
        pt.render_pass(0, 8)
        want = bits(pt.download()[0]).copy()
        rays = np.zeros(4, amber.api._RAY); rays["dir"][:, 2] = -1; rays["origin"][:, 2] = 3; rays["t_max"] = np.inf
        hits, occ = np.zeros(4, amber.api._RAY_HIT), np.zeros(4, np.uint8)
        for fn, out in ((lib.amber_hip_pt_cast_rays, hits), (lib.amber_hip_pt_occluded, occ)):
            for args in ((4, None, out.ctypes.data, amber.RAYS_HOST), (4, rays.ctypes.data, None, amber.RAYS_HOST), (4, rays.ctypes.data, out.ctypes.data, 2),
                         (4, rays.ctypes.data, out.ctypes.data, 0x80000001), ((1 << 31) + 1, rays.ctypes.data, out.ctypes.data, amber.RAYS_HOST)):
                assert fn(pt._h, *args) == -1, args                           # AMBER_EINVAL
                assert len(lib.amber_hip_last_error()) > 10
            assert fn(pt._h, 0, None, None, 0) == 0 and fn(pt._h, 0, None, None, amber.RAYS_HOST) == 0   # n == 0: AMBER_OK
            assert fn(pt._h, 4, rays.ctypes.data, out.ctypes.data, amber.RAYS_HOST) == 0
        pt.clear(); pt.render_pass(0, 8)
        assert np.array_equal(bits(pt.download()[0]), want)
        pt.close()


# ---- batch edges ---------------------------------------------------------------------------------------------------------------------------
# Where the kernels count: bvh_query_kernel's claim of the last block of 256 (n - base < 256), its ballot refill with fewer rays than lanes,
# ray_query_kernel's clamped tail lane, and AMBER_RAYS_HOST's trips through staging buffers that cast (32 bytes a ray) and occluded (1 byte) share.
SMALL_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 513)
STAGE_RAYS = 1 << 20                                                         # ray_query.inc: kQueryStageRays
TRIP_COUNTS = (STAGE_RAYS - 1, STAGE_RAYS, STAGE_RAYS + 1, 2 * STAGE_RAYS, 2 * STAGE_RAYS + 257)
N_TILE = 100_003                                                             # a prime: the trip boundary falls at another phase of the tiling each trip
GUARD, SENTINEL = 64, 0xA5


def mixed_t_max(t_oracle):
    """t_max by position: INFINITY, the number below the hit distance (a miss), NaN (a miss), INFINITY, half the hit distance (a miss), NaN, ..."""
    known = np.where(np.isnan(t_oracle), F32(1.0), t_oracle).astype(F32)
    tm = np.full(len(t_oracle), np.inf, F32)
    tm[1::6] = np.nextafter(known, F32(-np.inf))[1::6]
    tm[4::6] = (F32(0.5) * known)[4::6]
    tm[2::3] = np.nan
    return tm


def head_order(obj_oracle, window=4096):
    """The head of the base rays (the engine's own path rays) in an order that alternates rays the oracle hits with rays it misses while both last:
    in a sparse scene the first hundreds of eye rays all miss, in a closed room all hit."""
    head = np.arange(min(window, len(obj_oracle)))
    hit, miss = head[obj_oracle[head] >= 0], head[obj_oracle[head] < 0]
    m = min(len(hit), len(miss))
    return np.concatenate([np.stack([hit[:m], miss[:m]], 1).ravel(), hit[m:], miss[m:]])


def pack_rays(amber, o, d, tm):
    packed = np.zeros(len(o), amber.api._RAY)
    packed["origin"], packed["dir"], packed["t_max"] = o, d, tm
    return packed


def guarded_queries(amber, pt, packed, n, first="cast", bufs=None):
    """cast_rays and occluded of packed[:n] through AMBER_RAYS_HOST, in the order given, into arrays with GUARD sentinel elements behind element n,
    which must come back untouched.  Returns (hits[:n], occluded[:n])."""
    lib = amber.load_library()
    hits, occ = bufs if bufs is not None else (np.empty(n + GUARD, amber.api._RAY_HIT), np.empty(n + GUARD, np.uint8))
    hits[:n + GUARD].view(np.uint8)[:] = SENTINEL
    occ[:n + GUARD] = SENTINEL
    calls = {"cast": lambda: lib.amber_hip_pt_cast_rays(pt._h, n, packed.ctypes.data, hits.ctypes.data, amber.RAYS_HOST),
             "occluded": lambda: lib.amber_hip_pt_occluded(pt._h, n, packed.ctypes.data, occ.ctypes.data, amber.RAYS_HOST)}
    for name in (first, "occluded" if first == "cast" else "cast"):
        assert calls[name]() == 0, (name, lib.amber_hip_last_error())
    assert (hits[n:n + GUARD].view(np.uint8) == SENTINEL).all() and (occ[n:n + GUARD] == SENTINEL).all(), "a query wrote behind its last ray"
    return hits[:n], occ[:n]


def check_batch(label, hits, occ, exp):
    """every ray: object and t bit for bit, a miss is -1 / NaN / zeros, occluded is the same rule"""
    rep, obj_e, t_e = exp
    b = lambda x: np.ascontiguousarray(x, F32).view(np.uint32)
    obj = np.ascontiguousarray(hits["object"])
    assert np.array_equal(obj, obj_e), (label, np.flatnonzero(obj != obj_e)[:8])
    assert np.array_equal(b(hits["t"])[rep], b(t_e)[rep]), label
    miss = ~rep
    assert np.isnan(hits["t"][miss]).all() and not hits["pos"][miss].any() and not hits["normal"][miss].any(), label
    assert np.array_equal(occ, rep.astype(np.uint8)), (label, np.flatnonzero(occ != rep)[:8])


SMALL_ENGINES = {"cornell": (("ENGINE_AUTO", False), ("ENGINE_TWO_PHASE", False), ("ENGINE_LIST", False), ("ENGINE_BVH", False), ("ENGINE_REFERENCE_BVH", False)),
                 "cornell20": (("ENGINE_AUTO", False),),                        # the grouped two-phase engine
                 "spheres": (("ENGINE_AUTO", False), ("ENGINE_AUTO", True))}    # engine BVH on the host's tree and on the device's


@pytest.mark.parametrize("key", ["cornell", "cornell20", "spheres"])
def test_batches_smaller_than_a_block_and_around_its_edges(amber, key):
    c = _case(amber, key)
    for engine_name, device in SMALL_ENGINES[key]:
        engine = getattr(amber, engine_name)
        obj_o, t_o = c.oracle[O.ACCEL_BVH if engine == amber.ENGINE_REFERENCE_BVH else O.ACCEL_LIST]
        pt = c.tracer(engine, device)
        if key == "spheres":
            assert pt.build_info()["where"] == (amber.BUILD_DEVICE if device else amber.BUILD_HOST)
        head = head_order(obj_o)
        tm = mixed_t_max(t_o[head])                                             # by position in the batch: a batch is a prefix of the largest one
        for n in SMALL_COUNTS:
            k = head[:n]
            exp = expected(obj_o[k], t_o[k], tm[:n])
            assert n < 8 or (exp[0].any() and not exp[0].all())                # hits and misses
            hits, occ = guarded_queries(amber, pt, pack_rays(amber, c.org[k], c.dirs[k], tm[:n]), n, first="cast" if n % 2 else "occluded")
            check_batch(f"{c.name}, {engine_name}{', device tree' if device else ''}, {n} rays", hits, occ, exp)
        pt.close()


def tile_base(c):
    """N_TILE oracle-checked rays of the case (List semantics): its base rays, and as many more towards its objects as it takes"""
    if not hasattr(c, "tile"):
        org, dirs, (obj_o, t_o) = c.org, c.dirs, c.oracle[O.ACCEL_LIST]
        more = N_TILE - len(org)
        if more > 0:
            rng = np.random.default_rng(29)
            lo, hi, _ = scene_box(c.arr)
            o = rng.uniform(lo, hi, (more, 3))
            d = c.arr["p"][rng.integers(0, len(c.arr), more), :3] + rng.normal(size=(more, 3)) * 0.02 - o
            o, d = np.ascontiguousarray(o, F32), np.ascontiguousarray(d / np.linalg.norm(d, axis=1, keepdims=True), F32)
            io, to = c.osc.cast_many(o, d, O.ACCEL_LIST, threads=16)
            org, dirs, obj_o, t_o = np.concatenate([org, o]), np.concatenate([dirs, d]), np.concatenate([obj_o, io]), np.concatenate([t_o, to])
        c.tile = tuple(x[:N_TILE] for x in (org, dirs, obj_o, t_o))
    return c.tile


@pytest.mark.parametrize("key,engine_name", [("spheres", "ENGINE_AUTO"), ("cornell", "ENGINE_LIST"), ("cornell", "ENGINE_TWO_PHASE")])
def test_host_pointer_calls_of_one_two_and_three_staging_trips(amber, key, engine_name):
    """ray[i] = base[i % 100 003]: the expectation is tiled the same way and costs the oracle 10^5 rays.  One handle answers every count with occluded
    first (its output buffer grows from 1 byte a ray to 32), a second one with cast first and the counts from the largest down; each then answers 65 rays."""
    c = _case(amber, key)
    org, dirs, obj_o, t_o = tile_base(c)
    tm = mixed_t_max(t_o)
    exp = expected(obj_o, t_o, tm)
    assert exp[0].sum() > 10_000 and (~exp[0]).sum() > 10_000
    n_max = max(TRIP_COUNTS)
    idx = np.arange(n_max) % N_TILE
    packed = pack_rays(amber, org, dirs, tm)[idx]
    tiled = tuple(x[idx] for x in exp)
    bufs = (np.empty(n_max + GUARD, amber.api._RAY_HIT), np.empty(n_max + GUARD, np.uint8))
    for first, counts in (("occluded", TRIP_COUNTS), ("cast", TRIP_COUNTS[::-1])):
        pt = c.tracer(getattr(amber, engine_name))
        for n in counts + (65,):
            label = f"{c.name}, {engine_name}, {first} first, {n} rays"
            hits, occ = guarded_queries(amber, pt, packed, n, first, bufs)
            check_batch(label, hits, occ, tuple(x[:n] for x in tiled))
            records = hits.view(np.uint8).reshape(n, 32)                        # position and normal too: every trip repeats the first one's records
            assert np.array_equal(records, records[:N_TILE][idx[:n]]), label
        pt.close()


# ---- torch tensors, the device-pointer path, memory, the product library, speed: child processes (torch's runtime up before the engine's library) ------
TORCH_CHILD = r"""
import os, sys, json
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import torch
torch.cuda.init()
import amber_amd as A
from amber_amd import scenes
from test_update_objects import moved
from test_device_build import _objects, _random_rays
dev = torch.device("cuda", 0)
out = {{}}
kw = scenes.random_spheres(20_000, 7)
hs_a, hs_b = A.HostScene.create_arrays(**kw), A.HostScene.create_arrays(**moved(kw, 101))
rec = {{"A": _objects(hs_a), "B": _objects(hs_b)}}
o, d = _random_rays(rec["A"], 1_000_000, 17)
tm = np.random.default_rng(1).uniform(0.2, 3.0, len(o)).astype(np.float32); tm[::5] = np.inf; tm[1::50] = np.nan
same = lambda x, y: all(np.ascontiguousarray(p).tobytes() == np.ascontiguousarray(q).tobytes() for p, q in zip(x, y))
cpu = lambda ts: [t.cpu().numpy() for t in ts]
ident, batches = {{}}, {{}}
for name, hs, engine in (("bvh", hs_a, A.ENGINE_AUTO), ("cornell", A.HostScene.cornell_box(), A.ENGINE_AUTO), ("ref_bvh", hs_a, A.ENGINE_REFERENCE_BVH)):
    pt = A.PathTracer(hs, A.Sensor.default(64, 64), engine=engine)
    to, td, tt = (torch.from_numpy(x).to(dev) for x in (o, d, tm))
    ident[name] = []
    for stream in (None, torch.cuda.ExternalStream(pt.stream(), device=dev)):     # torch's current stream, then the handle's own
        if stream is None:
            got, occ = pt.cast_rays(to, td, tt), pt.occluded(to, td, tt)
        else:
            with torch.cuda.stream(stream):
                got, occ = pt.cast_rays(to, td, tt), pt.occluded(to, td, tt)
            stream.synchronize()
        ident[name].append(bool(same(cpu(got), pt.cast_rays(o, d, tm)) and np.array_equal(occ.cpu().numpy(), pt.occluded(o, d, tm))))
    for n in ((1 << 20) + 1, 257):                                               # two staging trips on the host side; a block and one ray
        k = np.arange(n) % len(o)
        o2, d2, t2 = o[k], d[k], tm[k]
        got, occ = pt.cast_rays(*(torch.from_numpy(x).to(dev) for x in (o2, d2, t2))), pt.occluded(*(torch.from_numpy(x).to(dev) for x in (o2, d2, t2)))
        batches.setdefault(name, []).append(bool(len(occ) == n and same(cpu(got), pt.cast_rays(o2, d2, t2)) and np.array_equal(occ.cpu().numpy(), pt.occluded(o2, d2, t2))))
    pt.close()
out["torch_equals_numpy"] = ident
out["device_pointer_batches"] = batches

# a query enqueued before an update answers for the old scene, one after it for the new scene (device pointers: nothing waits in between)
lib = A.load_library()
order = {{}}
for mode in (A.UPDATE_REFIT, A.UPDATE_REBUILD):
    pt = A.PathTracer(hs_a, A.Sensor.default(64, 64), flags=A.PT_FLAG_DEVICE_BUILD)
    ref = {{k: A.PathTracer(h, A.Sensor.default(64, 64)) for k, h in (("A", hs_a), ("B", hs_b))}}
    want = {{k: r.cast_rays(o, d, tm) for k, r in ref.items()}}
    ext = torch.cuda.ExternalStream(pt.stream(), device=dev)
    with torch.cuda.stream(ext):
        packed = torch.zeros((len(o), 8), dtype=torch.float32, device=dev)
        packed[:, 0:3], packed[:, 3], packed[:, 4:7] = torch.from_numpy(o).to(dev), torch.from_numpy(tm).to(dev), torch.from_numpy(d).to(dev)
        before, after = torch.empty((len(o), 8), dtype=torch.float32, device=dev), torch.empty((len(o), 8), dtype=torch.float32, device=dev)
        assert lib.amber_hip_pt_cast_rays(pt._h, len(o), packed.data_ptr(), before.data_ptr(), 0) == 0
        pt.update_flat(0, rec["B"], mode)
        assert lib.amber_hip_pt_cast_rays(pt._h, len(o), packed.data_ptr(), after.data_ptr(), 0) == 0
    ext.synchronize()
    split = lambda x: [x[:, 1].contiguous().view(torch.int32), x[:, 0].contiguous(), x[:, 2:5].contiguous(), x[:, 5:8].contiguous()]
    order[str(mode)] = [bool(same(cpu(split(before)), want["A"])), bool(same(cpu(split(after)), want["B"])), bool(not same(want["A"], want["B"]))]
    pt.close(); [r.close() for r in ref.values()]
out["order"] = order

# twenty queries of 1e6 rays: free device memory stays where the first one left it
growth = {{}}
for name, hs, engine in (("bvh", hs_a, A.ENGINE_AUTO), ("list", A.HostScene.cornell_box(), A.ENGINE_LIST)):
    pt = A.PathTracer(hs, A.Sensor.default(64, 64), engine=engine)
    free = []
    for k in range(20):
        pt.cast_rays(o, d, tm); pt.occluded(o, d, tm)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    pt.close()
    growth[name] = free
out["growth"] = growth
print("RESULT " + json.dumps(out))
"""


def _child(script, env=None, timeout=900, **fmt):
    p = subprocess.run([sys.executable, "-c", script.format(root=str(ROOT), **fmt)], capture_output=True, text=True, env=env, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][7:])


def test_torch_tensors_device_pointers_ordering_and_memory(amber):
    res = _child(TORCH_CHILD)
    print("\n" + json.dumps({k: v for k, v in res.items() if k != "growth"}))
    for name, flags in res["torch_equals_numpy"].items():
        assert flags == [True, True], name                                     # the device-pointer path and AMBER_RAYS_HOST: identical bytes
    assert set(res["device_pointer_batches"]) == {"bvh", "cornell", "ref_bvh"}
    for name, flags in res["device_pointer_batches"].items():
        assert flags == [True, True], name                                     # 2^20 + 1 and 257 rays through device pointers: the AMBER_RAYS_HOST bytes
    for mode, (old_scene, new_scene, scenes_differ) in res["order"].items():
        assert old_scene and new_scene and scenes_differ, mode
    for name, free in res["growth"].items():
        print(f"{name}: free device memory after queries 1 and 20: {free[0]} {free[19]}")
        assert len(free) == 20 and free[19] >= free[0], (name, free)


PRODUCT_CHILD = r"""
import os, sys, json
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import amber_amd as A
from amber_amd import scenes
from test_device_build import _objects, _random_rays
assert A.library_path().name == {lib!r} and A.is_lab() == {lab!r}
hs = A.HostScene.create_arrays(**scenes.random_spheres(20_000, 7))
o, d = _random_rays(_objects(hs), 200_000, 17)
tm = np.random.default_rng(1).uniform(0.2, 3.0, len(o)).astype(np.float32); tm[::5] = np.inf
for name, h, engine in (("bvh", hs, A.ENGINE_AUTO), ("cornell", A.HostScene.cornell_box(), A.ENGINE_AUTO), ("ref", hs, A.ENGINE_REFERENCE_BVH)):
    pt = A.PathTracer(h, A.Sensor.default(64, 64), engine=engine)
    obj, t, pos, nrm = pt.cast_rays(o, d, tm)
    np.savez(os.path.join({tmp!r}, name + ".npz"), obj=obj, t=t, pos=pos, nrm=nrm, occ=pt.occluded(o, d, tm))
    pt.close()
print("RESULT " + json.dumps(dict(ok=True)))
"""


def test_product_library_answers_with_the_lab_builds_bytes(amber, tmp_path):
    dirs = {}
    for lib, lab in (("libamber_hip.so", False), ("libamber_hip_lab.so", True)):
        dirs[lib] = tmp_path / lib
        dirs[lib].mkdir()
        _child(PRODUCT_CHILD, env=dict(os.environ, AMBER_AMD_LIB=lib), lib=lib, lab=lab, tmp=str(dirs[lib]))
    for name in ("bvh", "cornell", "ref"):
        a, b = (np.load(dirs[lib] / (name + ".npz")) for lib in dirs)
        assert (a["obj"] >= 0).sum() > 10_000
        for k in ("obj", "t", "pos", "nrm", "occ"):
            assert a[k].tobytes() == b[k].tobytes(), (name, k)


SPEED_CHILD = r"""
import os, sys, json
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import torch
torch.cuda.init()
import amber_amd as A
from amber_amd import scenes
assert A.is_lab()
dev = torch.device("cuda", 0)
W, H, n_paths, maxb, repeats = 1920, 1080, 420_000, 8, 4
hs = A.HostScene.create_arrays(**scenes.random_spheres(1_000_000, 7))
pt = A.PathTracer(hs, A.Sensor.default(W, H), seed=1)
rng = np.random.default_rng(3)
org, dirs = [], []
while sum(len(x) for x in org) < 1 << 20:
    px, sm = rng.integers(0, W * H, n_paths).astype(np.uint32), rng.integers(0, 256, n_paths).astype(np.uint32)
    eye = pt.kat_eye(px, sm)
    rec, casts = pt.kat_trace(px, sm, maxb)
    obj, pos = rec[:, :, 0].view(np.int32), rec[:, :, 2:5].view(np.float32)
    org.append(eye[:, 0:3]); dirs.append(eye[:, 3:6])
    for k in range(1, maxb):                              # the engine's own secondary rays: from one hit point towards the next
        ok = (obj[:, k - 1] >= 0) & (obj[:, k] >= 0) & (casts > k)
        o = pos[ok, k - 1]; d = pos[ok, k] - o
        ln = np.linalg.norm(d, axis=1, keepdims=True); keep = ln[:, 0] > 1e-6
        org.append(o[keep]); dirs.append((d[keep] / ln[keep]).astype(np.float32))
org, dirs = np.concatenate(org), np.concatenate(dirs)
perm = rng.permutation(len(org))[:1 << 20]
org, dirs = np.ascontiguousarray(org[perm], np.float32), np.ascontiguousarray(dirs[perm], np.float32)
n = len(org)
assert n == 1 << 20 and n * repeats >= 4_000_000
yard = []
for _ in range(3):
    yo, yt, ms = pt.kat_traversal_rate(org, dirs, waves=5, refill_min=16, repeats=repeats)
    yard.append(ms)
packed = np.zeros((n, 8), np.float32); packed[:, 0:3], packed[:, 3], packed[:, 4:7] = org, np.inf, dirs
rays = torch.from_numpy(np.tile(packed, (repeats, 1))).to(dev)        # the same rays in the same order, walked `repeats` times
hits = torch.empty((n * repeats, 8), dtype=torch.float32, device=dev)
occ = torch.empty(n * repeats, dtype=torch.uint8, device=dev)
lib = A.load_library()
ext = torch.cuda.ExternalStream(pt.stream(), device=dev)
torch.cuda.synchronize()
times = dict(cast=[], occluded=[])
with torch.cuda.stream(ext):
    for k in range(6):                                     # a warm-up, then five
        for name, call in (("cast", lambda: lib.amber_hip_pt_cast_rays(pt._h, n * repeats, rays.data_ptr(), hits.data_ptr(), 0)),
                           ("occluded", lambda: lib.amber_hip_pt_occluded(pt._h, n * repeats, rays.data_ptr(), occ.data_ptr(), 0))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ext); rc = call(); e1.record(ext); e1.synchronize()
            assert rc == 0
            if k: times[name].append(e0.elapsed_time(e1))
h = hits[:n].cpu().numpy()
got_obj, got_t = h[:, 1].copy().view(np.int32), h[:, 0]
hit = yo >= 0
answers = bool(np.array_equal(got_obj, yo) and np.array_equal(got_t[hit].view(np.uint32), yt[hit].view(np.uint32)) and np.array_equal(occ[:n].cpu().numpy() != 0, hit))
pt.close()
print("RESULT " + json.dumps(dict(n=n * repeats, yardstick_ms=yard, cast_ms=times["cast"], occluded_ms=times["occluded"], answers_equal=answers)))
"""


def test_cast_rays_keeps_up_with_the_traversal_only_kernel(amber):
    """The yardstick is the lab's traversal-only kernel (amber_hip_kat_traversal_rate, bvh_stream.inc) on the same rays, the same tree, the same waves
    per SIMD (5) and refill threshold (16): 2^20 eye and secondary rays of the 1M-sphere scene walked 4 times per launch (4.2 M rays).  cast_rays --
    timed with events on the handle's stream around the device-pointer call, best of 5 after a warm-up -- may take at most 1.15 x the yardstick's
    best_ms: the allowance for index resolution, ResolveHit and a 32-byte result in place of 8 bytes."""
    res = _child(SPEED_CHILD, timeout=1500)
    yard, cast, occ = min(res["yardstick_ms"]), min(res["cast_ms"]), min(res["occluded_ms"])
    print(f"\n{res['n']} rays: traversal-only kernel {yard:.3f} ms ({res['n'] / yard / 1e3:.0f} Mrays/s), cast_rays {cast:.3f} ms ({res['n'] / cast / 1e3:.0f} Mrays/s, "
          f"{cast / yard:.3f} x), occluded(INFINITY) {occ:.3f} ms ({res['n'] / occ / 1e3:.0f} Mrays/s)")
    assert res["answers_equal"]
    assert cast <= 1.15 * yard, (cast, yard)

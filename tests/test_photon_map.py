"""amber_hip_pm_build / amber_hip_pm_gather on the GPU, compared on BYTES with tests/photon_map_reference.py (the header's definition restated in numpy;
test_photon_map_reference_cpu.py checks it against brute force and the analytic density): hand-made photon sets that sit on every edge the grid and
the selection have, real photons and eye-ray hits of the Cornell box on four engines, Phong, and every way the contract says the calls can be cut
up, refused or combined with the rest of the handle."""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import photon_map_reference as R
import photon_reference as P

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
F = np.float32
EINVAL = -1
INFO_KEYS = ("n_photons", "n_dropped", "dims", "n_doublings", "max_cell_count")


def make_photons(pos, seed=5):
    rng = np.random.default_rng(seed)
    ph = np.zeros(len(pos), P.PHOTON)
    ph["pos"] = pos
    d = rng.normal(size=(len(pos), 3))
    d[:, 2] = np.abs(d[:, 2]) * np.where(rng.random(len(pos)) < 0.9, 1, -1)     # most arrive from above the plane z = 0, some from below (fs = 0)
    ph["dir_out"] = (d / np.linalg.norm(d, axis=1)[:, None]).astype(F)
    ph["weight"] = rng.random((len(pos), 3), dtype=F)
    ph["object"], ph["path"], ph["bounce"] = -7, np.arange(len(pos)), 1            # never read
    return ph


def make_queries(pos, radius, obj, seed=6):
    rng = np.random.default_rng(seed)
    pos = np.asarray(pos, F).reshape(-1, 3)
    q = np.zeros(len(pos), R.QUERY)
    q["pos"], q["radius"], q["object"], q["normal"] = pos, radius, obj, (0, 0, 1)
    d = rng.normal(size=(len(pos), 3))
    d[:, 2] = np.abs(d[:, 2])
    q["dir_out"] = (d / np.linalg.norm(d, axis=1)[:, None]).astype(F)
    q["weight"] = (0.25 + rng.random((len(pos), 3))).astype(F)
    return q


def same_info(got, want):
    assert {k: got[k] for k in INFO_KEYS} == {k: want[k] for k in INFO_KEYS}
    for k in ("cell_size", "lo", "hi"):
        assert np.asarray(got[k], F).tobytes() == np.asarray(want[k], F).tobytes(), k
    assert got["build_ms"] >= 0


class Shared:
    """The Cornell box, its per-object materials, one handle on engine AUTO for the hand-made sets, and a cube of photons with its queries and their
    restated answers: made once, left unchanged."""

    def __init__(self, amber):
        self.hs = amber.HostScene.cornell_box()
        self.mats = R.materials_of(self.hs)
        self.lambert = int(np.flatnonzero((self.mats[0] == R.MAT_LAMBERTIAN) & (self.mats[1] > 0).all(axis=1))[0])      # a white wall: every channel reflects
        self.pt = amber.PathTracer(self.hs, amber.Sensor.default(64, 64), seed=21)
        rng = np.random.default_rng(11)
        self.cube = make_photons(rng.random((4096, 3), dtype=F))
        self.cube.setflags(write=False)
        self.cell = 0.0625
        self.map = R.Map(self.cube, self.cell)
        self.queries = make_queries(rng.random((130, 3), dtype=F), (0.05 + 0.15 * rng.random(130)).astype(F), self.lambert)
        self.queries.setflags(write=False)
        self.want = {(k, raw): R.gather(self.map, self.queries, k, raw, self.mats) for k, raw in ((0, False), (7, False), (7, True))}

    def check(self, photons, cell, queries, ks=(0,), raws=(False,), pt=None, mats=None):
        """Build on the device and in numpy: the same info; gather: the same bytes.  Returns (map, info, the last answer)."""
        pt = pt or self.pt
        info = pt.pm_build(photons, cell)
        m = R.Map(photons, cell)
        same_info(info, m.info)
        got = None
        for k in ks:
            for raw in raws:
                got = pt.pm_gather(queries, k=k, raw=raw)
                want = R.gather(m, queries, k, raw, mats or self.mats)
                assert got.tobytes() == want.tobytes(), (k, raw, np.flatnonzero((got.view(np.uint32).reshape(-1, 8) != want.view(np.uint32).reshape(-1, 8)).any(axis=1))[:8])
        return m, info, got


_shared = {}


@pytest.fixture(scope="module")
def S(amber):
    if "s" not in _shared:
        _shared["s"] = Shared(amber)
    return _shared["s"]


def test_the_entry_points_exist_in_both_libraries(amber):
    lib = amber.load_library()
    assert amber.is_lab() and all(hasattr(lib, n) for n in ("amber_hip_pm_build", "amber_hip_pm_gather", "amber_hip_pm_release", "amber_hip_kat_bsdf", "amber_hip_kat_pm_stage_ms"))
    code = ("import ctypes, json, sys; lib = ctypes.CDLL(sys.argv[1]); "
            "print(json.dumps([hasattr(lib, n) for n in ('amber_hip_pm_build', 'amber_hip_pm_gather', 'amber_hip_pm_release', 'amber_hip_kat_bsdf')]))")
    out = subprocess.run([sys.executable, "-c", code, str(amber.library_path().parent / "libamber_hip.so")], capture_output=True, text=True, check=True).stdout
    assert json.loads(out) == [True, True, True, False]                              # the product: the three calls, no lab hook
    assert all(hasattr(amber.PathTracer, n) for n in ("pm_build", "pm_gather", "pm_release"))


# ---- hand-made sets, bit for bit ---------------------------------------------------------------------------------------------------------------------
def test_random_cube(S):
    m, info, _ = S.check(S.cube, S.cell, S.queries, ks=(0, 7, 1), raws=(False, True))
    assert info["dims"] == (16, 16, 16) and info["n_doublings"] == 0 and info["n_dropped"] == 0
    n_in = S.want[(0, False)]["n_in_radius"]
    assert (n_in > 7).sum() > 60 and (n_in <= 7).sum() > 5 and (n_in == 0).sum() < 20          # both paths of the gather are taken


def test_photons_on_cell_boundaries_and_at_hi(S):
    """A lattice with the cell size for its pitch: every photon on a cell boundary, the last layer at hi.  Queries: random; exactly on a photon;
    outside the bounds on each side and far outside; a radius larger than the whole grid; a radius below one cell."""
    g = np.arange(9, dtype=F) * F(0.125)
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)          # 729 photons, lo = 0, hi = 1
    ph = make_photons(np.concatenate([pos, pos[::3]]))                              # some twice: equal distances inside a cell
    rng = np.random.default_rng(3)
    where = [rng.random((40, 3)), pos[[0, 364, 728]], pos[[5, 77]]]
    radius = [0.05 + 0.3 * rng.random(40), [0.2, 0.2, 0.2], [1e-3, 0.124]]
    for a in range(3):
        for side in (-0.07, 1.07):
            p = np.full(3, 0.5); p[a] = side
            where.append(p[None]); radius.append([0.2])
    where += [[[30.0, 0.5, 0.5]], [[-1e30, 0.5, 3e38]], [[0.5, 0.5, 0.5]], [[0.5, 0.5, 0.5]], [[0.4, 0.3, 0.2]]]
    radius += [[0.5], [1e30], [10.0], [1e25], [0.01]]
    q = make_queries(np.concatenate([np.asarray(w, np.float64).reshape(-1, 3) for w in where]), np.concatenate([np.asarray(r, np.float64) for r in radius]).astype(F), S.lambert)
    m, info, got = S.check(ph, 0.125, q, ks=(0, 5), raws=(False, True))
    assert info["dims"] == (9, 9, 9) and info["hi"] == (1.0, 1.0, 1.0) and info["max_cell_count"] == 2
    full = S.pt.pm_gather(q, k=0)
    assert full["n_in_radius"][-3] == full["n_in_radius"][-2] == len(ph) and full["n_in_radius"][-1] == 0 and full["n_in_radius"][-5] == 0 and full["n_in_radius"][41] >= 2


def test_all_photons_coincident(S):
    ph = make_photons(np.tile(np.array([[0.3, -0.2, 7.0]], F), (100, 1)))
    q = make_queries([[0.3, -0.2, 7.0], [0.3, -0.2, 7.05], [0.3, -0.2, 7.2], [5.0, 5.0, 5.0]], [0.1, 0.1, 0.1, 20.0], S.lambert)
    m, info, got = S.check(ph, 0.5, q, ks=(0, 1, 99, 100, 101), raws=(True,))
    assert info["dims"] == (1, 1, 1) and info["max_cell_count"] == 100 and list(got["n_in_radius"]) == [100, 100, 0, 100]
    one = S.pt.pm_gather(q, k=1, raw=True)
    assert list(one["n_used"]) == [1, 1, 0, 1] and one["r2_used"][0] == 0 and one["r2_used"][2] == F(0.1) * F(0.1)


def test_k_equal_to_n_n_minus_one_and_one(S):
    S.pt.pm_build(S.cube, S.cell)
    n_in = S.want[(0, False)]["n_in_radius"]
    i = int(np.argmax(n_in))
    N = int(n_in[i])
    assert N > 40
    for k in (N, N - 1, 1):
        got = S.pt.pm_gather(S.queries, k=k)
        want = R.gather(S.map, S.queries, k, False, S.mats)
        assert got.tobytes() == want.tobytes(), k
        assert got["n_used"][i] == k and (got["r2_used"][i] == S.queries["radius"][i] * S.queries["radius"][i]) == (k == N)


def test_ties_at_the_kth_distance_follow_the_visit_order(S):
    """The octant set of test_photon_map_reference_cpu.py (eight tied photons and one nearer, k = 4), and three tied at the k-th distance behind one
    nearer photon with k = 2 and k = 3: which of them are used shows in the raw sum, since every photon has a weight of its own."""
    ph = make_photons(np.zeros((9, 3), F))
    ph["pos"][:8] = [(x, y, z) for x in (0.125, -0.125) for y in (-0.125, 0.125) for z in (0.125, -0.125)]
    ph["dir_out"], ph["weight"] = (0, 0, 1), (2.0 ** np.arange(9))[:, None]
    q = make_queries([[0, 0, 0]], [1.0], S.lambert)
    for cell, who in ((1.0, [0, 1, 2, 8]), (0.125, [5, 1, 7, 8])):
        m, info, got = S.check(ph, cell, q, ks=(4,), raws=(True,))
        assert got["n_used"][0] == 4 and got["n_in_radius"][0] == 9 and got["r2_used"][0] == F(3 * 0.125 ** 2)
        assert list(R.gather_one(m, q[0], 4, True, S.mats)[4]) == who
    three = make_photons(np.array([[0.5, 0, 0], [0, 0.5, 0], [0.01, 0, 0], [-0.5, 0, 0], [0.9, 0, 0]], F))
    for cell in (4.0, 0.25):
        for k in (2, 3):
            m, info, got = S.check(three, cell, q, ks=(k,), raws=(True, False))
            assert got["n_used"][0] == k and got["n_in_radius"][0] == 5 and got["r2_used"][0] == F(0.25)


def test_every_zero_result_condition(S):
    q = make_queries(np.full((12, 3), 0.5), 0.2, S.lambert)
    q["pos"][0, 1], q["pos"][1, 0], q["pos"][2, 2] = np.nan, np.inf, -np.inf
    q["radius"][3:8] = [np.nan, np.inf, 0.0, -0.0, -0.2]
    q["object"][8:11] = [-1, len(S.mats[0]), 2 ** 31 - 1]
    m, info, got = S.check(S.cube, S.cell, q, ks=(0, 3), raws=(False, True))
    assert not got[:11].view(np.uint32).any() and got["n_in_radius"][11] > 3 and got["rgb"][11].all()


def test_photons_with_nan_positions_are_dropped(S):
    ph = S.cube[:1000].copy()
    bad = np.arange(0, 1000, 37)
    ph["pos"][bad[0::3], 0], ph["pos"][bad[1::3], 1], ph["pos"][bad[2::3], 2] = np.nan, np.inf, -np.inf
    m, info, got = S.check(ph, S.cell, S.queries, ks=(0, 4))
    assert info["n_dropped"] == len(bad) and info["n_photons"] == 1000
    rest = np.delete(ph, bad)
    info2 = S.pt.pm_build(rest, S.cell)
    assert info2["n_dropped"] == 0 and {k: info2[k] for k in ("dims", "lo", "hi", "cell_size", "max_cell_count")} == {k: info[k] for k in ("dims", "lo", "hi", "cell_size", "max_cell_count")}
    assert S.pt.pm_gather(S.queries, k=4).tobytes() == got.tobytes()


def test_an_empty_map_answers_zeros(S):
    nothing = S.cube[:5].copy()
    nothing["pos"][:, 0] = np.nan
    for ph in (S.cube[:0], nothing):
        m, info, got = S.check(ph, 0.5, S.queries[:70])
        assert info["dims"] == (0, 0, 0) and info["cell_size"] == 0.5 and not got.view(np.uint32).any()


def test_a_small_cell_size_doubles(S):
    for cell in (1e-6, 3e-3, 1e-30):
        m, info, got = S.check(S.cube, cell, S.queries, ks=(0, 7))
        assert info["n_doublings"] > 0 and max(info["dims"]) <= 1024 and int(np.prod(info["dims"], dtype=np.int64)) <= 1 << 22
    flat = S.cube.copy()
    flat["pos"][:, 2] = 0.25
    m, info, got = S.check(flat, 1e-4, S.queries[:40])                               # 1024 cells per axis: the per-axis limit decides
    assert info["dims"][2] == 1 and max(info["dims"]) > 512
    assert got.tobytes() != S.want[(0, False)][:40].tobytes()


def test_counts_of_queries_and_splitting(S):
    """1, 63, 64 and 65 queries; a list equals its two halves: the answer to a query does not depend on the batch."""
    S.pt.pm_build(S.cube, S.cell)
    for key in ((0, False), (7, False), (7, True)):
        want = S.want[key]
        assert S.pt.pm_gather(S.queries, k=key[0], raw=key[1]).tobytes() == want.tobytes()
        for n in (1, 63, 64, 65):
            assert S.pt.pm_gather(S.queries[:n], k=key[0], raw=key[1]).tobytes() == want[:n].tobytes(), n
        a, b = S.pt.pm_gather(S.queries[:59], k=key[0], raw=key[1]), S.pt.pm_gather(S.queries[59:], k=key[0], raw=key[1])
        assert a.tobytes() + b.tobytes() == want.tobytes()
    assert S.pt.pm_gather(S.queries[:0]).shape == (0,)


# ---- real photons ------------------------------------------------------------------------------------------------------------------------------------
class Cornell:
    """Two DIFFUSE passes of the 64 x 64 Cornell box.  Queries: the first hits of a quarter of its eye rays (the walls, the boxes; a miss is a query with
    object -1), of every eye ray that ends on a light, and up to 32 vertices of the same light paths on a light: made on engine AUTO once, answered by
    the restatement once."""

    def __init__(self, amber, S):
        pt = S.pt
        self.photons, self.pinfo = pt.lt_trace_photons(0, 2, amber.PHOTON_DIFFUSE)
        pix = np.arange(64 * 64, dtype=np.uint32)
        eye = pt.kat_eye(pix, np.zeros(len(pix), np.uint32))
        obj, t, pos, nrm = pt.cast_rays(eye[:, 0:3] + eye[:, 3:6] * F(1e-3), eye[:, 3:6])       # (from just in front of the aperture blade the ray starts on)
        on_light = (obj >= 0) & (S.mats[0][np.clip(obj, 0, None)] == 4)
        keep = np.flatnonzero((pix % 4 == 0) | on_light)                                         # a quarter of the pixels, and every pixel that sees a light
        obj, pos, nrm, d_out = obj[keep], pos[keep], nrm[keep], -eye[keep, 3:6]
        lights, _ = pt.lt_trace_photons(0, 2, amber.PHOTON_LIGHT)                                # and where light paths come back to a light: queries on it for certain
        lights = lights[:32]
        obj, pos, nrm, d_out = (np.concatenate(p) for p in ((obj, lights["object"]), (pos, lights["pos"]), (nrm, lights["normal"]), (d_out, lights["dir_out"])))
        q = np.zeros(len(obj), R.QUERY)
        q["pos"], q["normal"], q["object"], q["dir_out"], q["weight"] = pos, nrm, obj, d_out, (1, 1, 1)
        extent = (self.photons["pos"].max(axis=0) - self.photons["pos"].min(axis=0)).max()
        self.radius = F(extent * 0.08)
        q["radius"] = self.radius
        self.queries = q
        self.cell = float(self.radius)
        self.map = R.Map(self.photons, self.cell)
        self.want = {(k, raw): R.gather(self.map, q, k, raw, S.mats) for k, raw in ((0, False), (16, False), (16, True))}
        self.kinds = S.mats[0][np.clip(obj, 0, None)]
        self.obj = obj


@pytest.fixture(scope="module")
def CB(amber, S):
    if "cb" not in _shared:
        _shared["cb"] = Cornell(amber, S)
    return _shared["cb"]


def test_the_cornell_inputs_cover_what_they_should(CB):
    n_in = CB.want[(0, False)]["n_in_radius"]
    print(f"\n{len(CB.photons)} photons, {len(CB.queries)} queries, radius {CB.radius}, dims {CB.map.info['dims']}, in radius: median {np.median(n_in)}, max {n_in.max()}")
    assert len(CB.photons) > 4000 and (CB.kinds[CB.obj >= 0] == 4).sum() >= 2 and (CB.kinds[CB.obj >= 0] == R.MAT_LAMBERTIAN).sum() > 300
    assert (n_in > 16).sum() > 300 and ((n_in > 0) & (n_in <= 16)).sum() > 5        # both paths of the gather
    lit = CB.want[(0, False)]["rgb"][(CB.obj >= 0) & (CB.kinds == R.MAT_LAMBERTIAN)]
    assert (lit > 0).any(axis=1).mean() > 0.7
    assert not CB.want[(0, False)]["rgb"][(CB.obj >= 0) & (CB.kinds == 4)].any()            # a light is no diffuse surface: fs = 0


ENGINES = ["ENGINE_AUTO", "ENGINE_LIST", "ENGINE_BVH", "ENGINE_REFERENCE_BVH"]


@pytest.mark.parametrize("engine", ENGINES)
def test_real_photons_on_every_engine(amber, S, CB, engine):
    pt = amber.PathTracer(S.hs, amber.Sensor.default(64, 64), seed=21, engine=getattr(amber, engine))
    if engine != "ENGINE_REFERENCE_BVH":                                            # (that engine follows the reference's tree on ties: its own list may differ)
        own, _ = pt.lt_trace_photons(0, 2, amber.PHOTON_DIFFUSE)
        assert own.tobytes() == CB.photons.tobytes()
    same_info(pt.pm_build(CB.photons, CB.cell), CB.map.info)
    for (k, raw), want in CB.want.items():
        assert pt.pm_gather(CB.queries, k=k, raw=raw).tobytes() == want.tobytes(), (k, raw)
    pt.close()


# ---- Phong -------------------------------------------------------------------------------------------------------------------------------------------
def phong_inputs(amber):
    hs = amber.HostScene.create(**P.SCENE)
    mats = R.materials_of(hs)
    return hs, mats, [int(i) for i in np.flatnonzero(mats[0] == R.MAT_PHONG)]


def test_phong_bit_for_bit(amber):
    if amber.math_mode() != amber.MATH_GLIBC:
        pytest.skip("the restatement's powf is glibc's; this library was built with the portable sin / cos / pow")
    hs, mats, phong = phong_inputs(amber)
    assert phong and {float(mats[2][i]) for i in phong} >= {20.0}
    rng = np.random.default_rng(8)
    ph = make_photons((rng.random((2000, 3)) * 0.5).astype(F), seed=9)
    pos = (rng.random((96, 3)) * 0.5).astype(F)
    q = make_queries(pos, 0.08, np.resize(phong, 96), seed=10)
    nrm = rng.normal(size=(96, 3))
    q["normal"] = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(F)
    q["dir_out"][:48] = q["normal"][:48]                                             # head-on: the lobe is wide open
    pt = amber.PathTracer(hs, amber.Sensor.default(16, 16))
    info = pt.pm_build(ph, 0.08)
    m = R.Map(ph, 0.08)
    same_info(info, m.info)
    for k, raw in ((0, True), (0, False), (5, True)):
        got, want = pt.pm_gather(q, k=k, raw=raw), R.gather(m, q, k, raw, mats)
        assert got.tobytes() == want.tobytes(), (k, raw)
    pt.close()
    assert (want["rgb"] > 0).all(axis=1).sum() > 40 and len(np.unique(want["rgb"][:, 0])) > 40


def test_the_bsdf_alone_against_binary64(amber):
    """amber_hip_kat_bsdf = rho * SymmetricBSDF for every material of photon_reference.SCENE, in the manner of test_f64_reference_gpu.py's Radiance: zero
    exactly where the binary64 product cos_o * cos_i is <= 0, outside the margin of a dot product's own rounding (2.5 ulp of 1 for three products and two
    sums of values <= 1, taken 4 x and 4 x again as there); zero for every kind that is not diffuse.  Elsewhere, within a bound from the operations.
    Lambertian: rho / pi through binary32 pi (0.5 ulp), one division and one product: 1.5 ulp.  Phong: (e + 2) / (2 pi) 2 ulp, the product with powf
    and with rho 1 ulp, powf itself 1 ulp, and the error of cos_alpha -- a reflection (three roundings per component of values <= 3) and a dot product:
    7 ulp of 1 -- grows by e / cos_alpha through the power; checked where cos_alpha >= 0.25.  Both taken 4 x."""
    import f64_reference as R64
    hs, mats, phong = phong_inputs(amber)
    kind, rho, param = mats
    rng = np.random.default_rng(12)
    n = 4096
    obj = rng.integers(0, len(kind), n).astype(np.int32)
    obj[: n // 2] = np.resize(phong, n // 2)
    nrm, do, di = (R64.unit(rng.normal(size=(n, 3))).astype(F) for _ in range(3))
    di[: n // 4] = (2 * R64.dot(do[: n // 4], nrm[: n // 4])[:, None] * nrm[: n // 4] - do[: n // 4] + 0.2 * rng.normal(size=(n // 4, 3))).astype(F)   # near the mirror direction
    di = R64.unit(di.astype(np.float64)).astype(F)
    pt = amber.PathTracer(hs, amber.Sensor.default(16, 16))
    got = pt.kat_bsdf(obj, nrm, do, di)
    with pytest.raises(amber.AmberError, match="object index out of range"):
        pt.kat_bsdf(np.array([len(kind)], np.int32), nrm[:1], do[:1], di[:1])
    pt.close()
    N, O_, I_ = nrm.astype(np.float64), do.astype(np.float64), di.astype(np.float64)
    cos_o, cos_i = R64.dot(O_, N), R64.dot(I_, N)
    margin = R64.MARGIN_FACTOR * R64.BOUND_FACTOR * 2.5 * 2.0 ** -23
    sure = (np.abs(cos_o) > margin) & (np.abs(cos_i) > margin)
    k = kind[obj]
    diffuse = (k == R.MAT_LAMBERTIAN) | (k == R.MAT_PHONG)
    assert not got[~diffuse].any() and (~diffuse).sum() > 200
    dark = diffuse & sure & (cos_o * cos_i < 0)
    assert dark.sum() > 500 and not got[dark].any()
    lit = diffuse & sure & (cos_o * cos_i > 0)
    lam = lit & (k == R.MAT_LAMBERTIAN)
    want = rho[obj].astype(np.float64) / np.pi
    assert lam.sum() > 50 and (np.abs(got[lam] - want[lam]) <= R64.BOUND_FACTOR * 1.5 * R64.ulp32(want[lam])).all()
    e = param[obj].astype(np.float64)
    cos_alpha = np.maximum(0.0, R64.dot(2 * cos_i[:, None] * N - I_, O_))
    ph = lit & (k == R.MAT_PHONG) & (cos_alpha >= 0.25)
    fs = (e + 2) / (2 * np.pi) * cos_alpha ** e
    want = rho[obj].astype(np.float64) * fs[:, None]
    rel = R64.BOUND_FACTOR * (4 + 7 * e / np.maximum(cos_alpha, 0.25)) * 2.0 ** -23
    assert ph.sum() > 300 and (np.abs(got[ph] - want[ph]) <= rel[ph, None] * want[ph] + 2.0 ** -149).all()
    if amber.math_mode() == amber.MATH_GLIBC:                                        # and the restatement's bits, every row
        for i in range(0, n, 7):
            f = R.symmetric_bsdf(int(kind[obj[i]]), param[obj[i]], nrm[i], do[i], di[i : i + 1])
            assert (rho[obj[i]] * f[0]).tobytes() == got[i].tobytes(), i


# ---- build, release, order of the input ----------------------------------------------------------------------------------------------------------------
def test_a_second_build_replaces_the_first_and_release_ends_the_map(amber, S):
    pt = amber.PathTracer(S.hs, amber.Sensor.default(16, 16))
    other = make_photons(np.random.default_rng(4).random((777, 3), dtype=F) * F(0.5), seed=14)
    want_other = R.gather(R.Map(other, 0.1), S.queries, 7, False, S.mats)
    assert want_other.tobytes() != S.want[(7, False)].tobytes()
    for _ in range(2):
        pt.pm_build(S.cube, S.cell)
        assert pt.pm_gather(S.queries, k=7).tobytes() == S.want[(7, False)].tobytes()
        pt.pm_build(other, 0.1)
        assert pt.pm_gather(S.queries, k=7).tobytes() == want_other.tobytes()
    pt.pm_release()
    with pytest.raises(amber.AmberError, match="has no photon map"):
        pt.pm_gather(S.queries, k=7)
    pt.pm_release()                                                                  # releasing nothing is fine
    pt.pm_build(S.cube, S.cell)
    assert pt.pm_gather(S.queries, k=7).tobytes() == S.want[(7, False)].tobytes()
    pt.close()


def test_a_permuted_input_changes_only_the_order_of_the_sum(S):
    perm = np.random.default_rng(15).permutation(len(S.cube))
    shuffled = S.cube[perm]
    m, info, got = S.check(shuffled, S.cell, S.queries, ks=(7,))
    want = S.want[(7, False)]
    for name in ("n_used", "n_in_radius", "r2_used"):
        assert np.array_equal(got[name], want[name]), name
    assert np.allclose(got["rgb"], want["rgb"], rtol=1e-4) and got["rgb"].tobytes() != want["rgb"].tobytes()


# ---- pointer modes, the product library ----------------------------------------------------------------------------------------------------------------
CHILD = r"""
import json, os, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np
if {device!r}:
    import torch                                                 # (before the library: torch brings its own HIP runtime)
import amber_amd as A
assert A.library_path().name == {lib!r}
ph, q = np.load(os.path.join({tmp!r}, "photons.npy")), np.load(os.path.join({tmp!r}, "queries.npy"))
pt = A.PathTracer(A.HostScene.cornell_box(), A.Sensor.default(64, 64), seed=21)
res = dict(lab=A.is_lab())
if {device!r}:
    dph = torch.from_numpy(ph.view(np.float32).reshape(-1, 16).copy()).cuda()
    dq = torch.from_numpy(q.view(np.float32).reshape(-1, 16).copy()).cuda()
    info = pt.pm_build(dph, {cell!r})
    dph.zero_()                                                  # the map keeps its own copy
    torch.cuda.synchronize()
    for k, raw in ((0, False), (7, False), (7, True)):
        out = pt.pm_gather(dq, k=k, raw=raw)
        np.save(os.path.join({tmp!r}, "out_%d_%d.npy" % (k, raw)), out.cpu().numpy())
    bad = []
    for call in (lambda: pt.pm_build((dph.data_ptr() + 4, 10), {cell!r}), lambda: pt.pm_gather(dq.view(-1)[1:1 + 16 * 4].view(4, 16)),
                 lambda: pt.pm_gather(dq[:4], out=torch.empty(4 * 8 + 1, device="cuda")[1:].view(4, 8))):
        try:
            call(); bad.append("accepted")
        except A.AmberError as e:
            bad.append("16-byte aligned" in str(e))
    res["misaligned"] = bad
    res["good_after"] = bool((pt.pm_gather(dq, k=7).cpu().numpy() == np.load(os.path.join({tmp!r}, "out_7_0.npy"))).all())
else:
    info = pt.pm_build(ph, {cell!r})
    for k, raw in ((0, False), (7, False), (7, True)):
        np.save(os.path.join({tmp!r}, "out_%d_%d.npy" % (k, raw)), pt.pm_gather(q, k=k, raw=raw).view(np.float32).reshape(-1, 8))
res["dims"] = list(info["dims"])
pt.close()
print("RESULT " + json.dumps(res))
"""


def _child(tmp_path, S, lib, device):
    np.save(tmp_path / "photons.npy", S.cube)
    np.save(tmp_path / "queries.npy", S.queries)
    script = CHILD.format(root=str(ROOT), tests=str(ROOT / "tests"), tmp=str(tmp_path), lib=lib, device=device, cell=S.cell)
    p = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=dict(os.environ, AMBER_AMD_LIB=lib), timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    assert res["dims"] == [16, 16, 16]
    for (k, raw), want in S.want.items():
        assert np.load(tmp_path / f"out_{k}_{int(raw)}.npy").tobytes() == want.tobytes(), (lib, device, k, raw)
    return res


def test_device_pointers_give_the_host_modes_bytes(S, tmp_path):
    res = _child(tmp_path, S, "libamber_hip_lab.so", True)
    assert res["lab"] and res["misaligned"] == [True, True, True] and res["good_after"]


def test_the_product_library_gives_the_lab_librarys_bytes(S, tmp_path):
    assert not _child(tmp_path, S, "libamber_hip.so", False)["lab"]


# ---- refusals, side effects ------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_next_good_call_unchanged(amber, S):
    lib = amber.load_library()
    pt = amber.PathTracer(S.hs, amber.Sensor.default(16, 16))
    ph, q = np.array(S.cube), np.array(S.queries)
    out = np.zeros(len(q), amber.GATHER_RESULT_DTYPE)
    fresh = np.array(out)
    dev = pt.device_framebuffer()[0]                                                  # some device address: a refused call does not look behind it
    HOST, RAW = amber.api.RAYS_HOST, amber.PM_RAW_SUM
    nan, inf = float("nan"), float("inf")

    def build(h, p, n, cell, flags):
        info = amber.PhotonMapInfo(n_photons=9, n_dropped=9, cell_size=9.0)
        rc = lib.amber_hip_pm_build(h, p, n, cell, flags, C.byref(info))
        assert rc == 0 or bytes(info) == bytes(amber.PhotonMapInfo())                   # zeroed first, whatever the answer
        return rc

    def gather(h, n, qp, op, k, flags):
        return lib.amber_hip_pm_gather(h, n, qp, op, k, flags)

    def good():
        assert pt.pm_gather(q, k=7).tobytes() == S.want[(7, False)].tobytes()

    with pytest.raises(amber.AmberError, match="has no photon map"):                  # gather before any build
        pt.pm_gather(q, k=7)
    assert gather(pt._h, 0, None, None, 0, HOST) == EINVAL                            # ... also with nothing to do
    pt.pm_build(ph, S.cell)
    good()
    P_, Q_, O_, n, nq = ph.ctypes.data, q.ctypes.data, out.ctypes.data, len(ph), len(q)
    refusals = {
        "build: null handle": lambda: build(None, P_, n, S.cell, HOST),
        "build: null photons with a count": lambda: build(pt._h, None, n, S.cell, HOST),
        "build: n > 2^31": lambda: build(pt._h, P_, (1 << 31) + 1, S.cell, HOST),
        "build: cell_size NaN": lambda: build(pt._h, P_, n, nan, HOST),
        "build: cell_size inf": lambda: build(pt._h, P_, n, inf, HOST),
        "build: cell_size 0": lambda: build(pt._h, P_, n, 0.0, HOST),
        "build: cell_size < 0": lambda: build(pt._h, P_, n, -0.5, HOST),
        "build: unknown flag bits": lambda: build(pt._h, P_, n, S.cell, HOST | 2),
        "build: misaligned device pointer": lambda: build(pt._h, dev + 8, 4, S.cell, 0),
        "gather: null handle": lambda: gather(None, nq, Q_, O_, 7, HOST),
        "gather: null queries": lambda: gather(pt._h, nq, None, O_, 7, HOST),
        "gather: null output": lambda: gather(pt._h, nq, Q_, None, 7, HOST),
        "gather: n > 2^31": lambda: gather(pt._h, (1 << 31) + 1, Q_, O_, 7, HOST),
        "gather: k > 2^31": lambda: gather(pt._h, nq, Q_, O_, (1 << 31) + 1, HOST),
        "gather: unknown flag bits": lambda: gather(pt._h, nq, Q_, O_, 7, HOST | RAW | 4),
        "gather: misaligned queries": lambda: gather(pt._h, 1, dev + 8, dev + 4096, 7, 0),
        "gather: misaligned output": lambda: gather(pt._h, 1, dev, dev + 4096 + 4, 7, 0),
        "release: null handle": lambda: lib.amber_hip_pm_release(None),
    }
    for name, call in refusals.items():
        assert call() == EINVAL, name
        assert lib.amber_hip_last_error(), name
        assert out.tobytes() == fresh.tobytes(), name
        good()
    huge = np.array(ph[:4])
    huge["pos"][0, 0], huge["pos"][1, 0] = -3e38, 3e38                                # an extent that overflows binary32: no cell size covers it
    assert build(pt._h, huge.ctypes.data, 4, S.cell, HOST) == EINVAL and b"overflows" in lib.amber_hip_last_error()
    good()
    assert gather(pt._h, 0, None, None, 7, HOST) == 0                                 # AMBER_OK with nothing written
    assert lib.amber_hip_pm_build(pt._h, P_, n, S.cell, HOST, None) == 0              # info may be NULL
    good()
    pt.pm_release()
    assert gather(pt._h, nq, Q_, O_, 7, HOST) == EINVAL and out.tobytes() == fresh.tobytes()
    pt.close()


def test_framebuffer_ray_counter_and_kernel_time_are_left_alone(amber, S):
    pt, fresh = amber.PathTracer(S.hs, amber.Sensor.default(32, 32), seed=3), amber.PathTracer(S.hs, amber.Sensor.default(32, 32), seed=3)
    pt.render_pass(0, 4)
    img, rays = pt.download()
    before = (img.tobytes(), rays, pt.kernel_time())
    pt.pm_build(S.cube, S.cell)
    assert pt.pm_gather(S.queries, k=7).tobytes() == S.want[(7, False)].tobytes()
    img, rays = pt.download()
    assert rays > 0 and (img.tobytes(), rays, pt.kernel_time()) == before
    pt.render_pass(4, 4)
    assert pt.pm_gather(S.queries, k=7).tobytes() == S.want[(7, False)].tobytes()     # the map outlives a render pass
    fresh.render_pass(0, 4); fresh.render_pass(4, 4)
    (a, ra), (b, rb) = pt.download(), fresh.download()
    assert a.tobytes() == b.tobytes() and ra == rb > rays
    build_ms, gather_ms = pt.kat_pm_stage_ms()                                        # switches the timing on
    pt.pm_build(S.cube, S.cell)
    assert pt.pm_gather(S.queries, k=7).tobytes() == S.want[(7, False)].tobytes()
    build_ms, gather_ms = pt.kat_pm_stage_ms()
    assert build_ms > 0 and gather_ms > 0 and pt.kat_pm_stage_ms() == (0.0, 0.0)
    pt.close(); fresh.close()

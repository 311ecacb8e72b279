"""tests/photon_map_reference.py -- the numpy restatement the GPU tests compare amber_hip_pm_gather with bit for bit -- checked on its own, without a GPU:
its used set against a brute-force k-nearest in binary64 over all photons, its in-radius count against a binary32 brute force (the cell range loses
nothing), and its density estimate against the analytic answer (a wrong pi or kernel normalisation, which a bit-exact comparison with a restatement
that shares the mistake cannot see)."""
import numpy as np
import pytest

import photon_map_reference as R
import photon_reference as P

F = np.float32
N_PHOTONS, N_QUERIES = 4096, 1024
LAMBERT = (np.array([R.MAT_LAMBERTIAN], np.uint32), np.array([[0.5, 0.6, 0.7]], F), np.array([0.0], F))       # one object, one Lambertian material


def random_set(seed):
    rng = np.random.default_rng(seed)
    ph = np.zeros(N_PHOTONS, P.PHOTON)
    ph["pos"] = rng.random((N_PHOTONS, 3), dtype=F)                              # the unit cube
    ph["dir_out"] = (0, 0, 1)
    ph["weight"] = rng.random((N_PHOTONS, 3), dtype=F)
    q = np.zeros(N_QUERIES, R.QUERY)
    q["pos"] = rng.random((N_QUERIES, 3), dtype=F)
    q["radius"] = (0.05 + 0.15 * rng.random(N_QUERIES)).astype(F)                # 0.05 .. 0.2
    q["normal"], q["dir_out"], q["weight"] = (0, 0, 1), (0, 0, 1), (1, 1, 1)
    return ph, q


_sets = {}


@pytest.fixture(scope="module", params=[1, 2])
def data(request):
    if request.param not in _sets:
        ph, q = random_set(request.param)
        _sets[request.param] = (ph, q, R.Map(ph, 0.0625))
    return _sets[request.param]


def test_the_used_set_is_the_binary64_k_nearest_set(data):
    """k in {0, 1, 7, N, N - 1} per query (N its own in-radius count; N - 1 below 0 is taken as 0, the uncapped case).  A case the brute force classifies
    as fragile -- a d2 within 4 binary32 ulp of r2, or the k-th and (k + 1)-th distance within 4 ulp: a tie at the k-th distance at binary32
    resolution -- may differ and is skipped; at most 1 % of the cases may be."""
    ph, queries, m = data
    assert m.info["dims"] == (16, 16, 16) or max(m.info["dims"]) == 16
    cases = skipped = cut = 0
    for q in queries:
        n = R.brute_knn_f64(ph, q, 0)[1]
        for k in (0, 1, 7, n, max(n - 1, 0)):
            want, n64, fragile = R.brute_knn_f64(ph, q, k)
            cases += 1
            if fragile:
                skipped += 1
                continue
            _, n_used, r2_used, n_in, used = R.gather_one(m, q, k, True, LAMBERT)
            assert n_in == n64 and n_used == len(want) == (n_in if k == 0 or n_in <= k else k)
            assert np.array_equal(np.sort(used), want)
            if k and n_in > k:
                cut += 1
                assert r2_used < q["radius"] * q["radius"]
    print(f"\n{cases} cases, {skipped} skipped as fragile, {cut} cut by k")
    assert cases == 5 * N_QUERIES and skipped <= cases // 100 and cut > N_QUERIES


def test_the_cell_range_loses_no_photon(data):
    """k = 0: n_in_radius equals a binary32 brute force over ALL photons with the same d2 and the same test.  No case is skipped: cellf is monotone and
    pos - radius is correctly rounded, so a photon with d2 < r2 lies in a visited cell."""
    ph, queries, m = data
    total = 0
    for q in queries:
        n_in = R.gather_one(m, q, 0, True, LAMBERT)[3]
        assert n_in == R.brute_count_f32(ph, q)
        total += n_in
    assert total > 10 * N_QUERIES


def test_queries_at_and_beyond_the_bounds_lose_nothing_either():
    ph, _ = random_set(3)
    m = R.Map(ph, 0.0625)
    q = np.zeros(1, R.QUERY)
    q["normal"], q["dir_out"], q["weight"] = (0, 0, 1), (0, 0, 1), (1, 1, 1)
    for pos, radius in (((-0.05, 0.5, 0.5), 0.1), ((1.04, 1.04, 1.04), 0.2), ((0.5, 0.5, 0.5), 5.0), ((0.5, -3.0, 0.5), 0.5), ((1e30, 0.5, 0.5), 0.5),
                        (tuple(m.hi), 0.01), (tuple(m.lo), 0.01)):
        q["pos"], q["radius"] = pos, radius
        assert R.gather_one(m, q[0], 0, True, LAMBERT)[3] == R.brute_count_f32(ph, q[0]), (pos, radius)


def test_ties_are_decided_by_visit_order():
    """Eight photons at the same distance of the origin, one per octant (input index 0 .. 7, x outermost), and one at the origin (index 8); k = 4 takes
    the origin's and three of the tied ones.  One cell: the first three in input order.  One cell per octant: the first three in z, then y, then x."""
    ph = np.zeros(9, P.PHOTON)
    ph["pos"][:8] = [(x, y, z) for x in (0.125, -0.125) for y in (-0.125, 0.125) for z in (0.125, -0.125)]
    ph["dir_out"], ph["weight"] = (0, 0, 1), np.arange(1, 10, dtype=F)[:, None]
    q = np.zeros(1, R.QUERY)
    q["radius"], q["normal"], q["dir_out"], q["weight"] = 1.0, (0, 0, 1), (0, 0, 1), (1, 1, 1)
    one = R.Map(ph, 1.0)
    assert one.info["dims"] == (1, 1, 1) and list(R.gather_one(one, q[0], 4, True, LAMBERT)[4]) == [0, 1, 2, 8]
    octants = R.Map(ph, 0.125)
    assert octants.info["dims"] == (3, 3, 3)
    rgb, n_used, r2_used, n_in, used = R.gather_one(octants, q[0], 4, True, LAMBERT)
    assert list(used) == [5, 1, 7, 8] and (n_used, n_in) == (4, 9) and r2_used == F(3 * 0.125 ** 2)
    assert np.allclose(rgb, (6 + 2 + 8 + 9) * LAMBERT[1][0] / np.pi, rtol=1e-6)              # the weights are index + 1


FLUX_SEEDS = range(8)
MEASURED_SPREAD = 0.0276      # standard deviation of estimate / exact over the eight seeds, as measured (0.02758); Poisson: 1 / sqrt(N in the disk) = 0.039


def plane_estimate(seed, n=16384, radius=0.1125, w=F(0.25)):
    rng = np.random.default_rng(seed)
    ph = np.zeros(n, P.PHOTON)
    ph["pos"][:, :2] = rng.random((n, 2), dtype=F)                               # uniform on the unit square of the plane z = 0
    ph["dir_out"], ph["weight"] = (0, 0, 1), w
    q = np.zeros(1, R.QUERY)
    q["pos"], q["radius"], q["normal"], q["dir_out"], q["weight"] = (0.5, 0.5, 0.0), radius, (0, 0, 1), (0.6, 0, 0.8), (1, 1, 1)
    rgb = R.gather_one(R.Map(ph, 0.05), q[0], 0, False, LAMBERT)[0]
    exact = LAMBERT[1][0].astype(np.float64) / np.pi * (n * float(w))            # rho / pi * flux per unit area (the square has area 1)
    return rgb.astype(np.float64) / exact


def test_density_estimate_of_a_uniformly_lit_plane():
    """16384 photons of weight 0.25 uniform on the unit square, a Lambertian query at its centre with radius 0.1125 (about 650 photons in the disk):
    rgb against rho / pi * flux density.  Tolerance: four times the spread over the eight seeds, measured as 0.0276 (the Poisson figure 1 / sqrt(650) is
    0.039; the largest deviation of a seed was 0.047): 0.110.  A missing or squared pi, a kernel over the sphere instead of the disk or a diameter for a radius are off by a factor of 2 at least."""
    ratios = np.array([plane_estimate(s) for s in FLUX_SEEDS])
    spread = ratios[:, 0].std()
    print(f"\nestimate / exact per seed: {np.round(ratios[:, 0], 4)}, spread {spread:.5f}")
    assert np.allclose(ratios, ratios[:, :1], rtol=1e-4)                         # the three channels see the same photons (650 binary32 additions each)
    assert np.abs(ratios - 1.0).max() <= 4 * MEASURED_SPREAD
    assert 0.5 * MEASURED_SPREAD < spread < 2 * MEASURED_SPREAD                  # the figure above is still what these inputs give

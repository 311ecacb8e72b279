"""The oracle against the binary64 statement of the same operations (tests/f64_reference.py) -- no GPU needed.

Bit parity proves that the kernels and the oracle are one function; these tests bound that function against the geometric and optical
definitions, on random inputs and on inputs aimed at the places where the answer changes (tests/f64_inputs.py).  Bounds: 4 x the
measured worst case of tests/golden/f64_reference_bounds.json; margins: 4 x the bounds.  A ray inside the margin of a boundary is
classified, not skipped: its answer must be one the binary64 reference gives on one side of that boundary.
"""
import numpy as np
import pytest

import f64_inputs as I
import f64_reference as R
import oracle_binding as O

BOUNDS = I.load_bounds()
RANDOM_CAP, MIXED_CAP, SIDE_SHARE = 0.02, 0.05, 0.30


def judged(name, scene_kw, o, d, answer):
    """The answers of some implementation for rays of the input set `name`, judged against the binary64 candidates with that set's bounds."""
    osc = O.Scene.create(**scene_kw)
    kinds, params = I.scene_arrays(osc)
    floor = R.BOUND_FACTOR * I.FLOOR_ULP                                  # a kind this set never hit (the blades of a single-primitive scene)
    b = {**{k: {"t": floor, "pos": floor, "normal": floor, "residual": floor} for k in R.KIND_NAMES}, **BOUNDS["intersect"][name]}
    c = R.with_radius(R.scene_candidates(kinds, params, o, d), kinds, params)
    return kinds, params, b, c, R.judge(c, *answer, b, o, d)


def check_intersections(name, scene_kw, o, d, aimed, answer, cap):
    """Shared with the GPU leg: `answer` = (object, t, pos, normal) of some implementation for the rays of one input set.
    cap: the largest ill-conditioned share of the random half."""
    kinds, params, b, c, j = judged(name, scene_kw, o, d, answer)
    obj, t, pos, nrm = answer
    well = j["well"]
    ill_random = float((~well[~aimed]).mean())
    side = float((j["ref_obj"][aimed] >= 0).mean())
    print(f"{name}: ill-conditioned {ill_random:.4f} of the random half (cap {cap}), {(~well[aimed]).mean():.3f} of the aimed half; aimed rays that hit in binary64: {side:.3f}; "
          f"worst t / pos / normal error on well-conditioned hits {j['err_t'][well].max():.2f} / {j['err_pos'][well].max():.2f} / {j['err_normal'][well].max():.2f} ulp")
    # hit / miss and object: the binary64 answer on every well-conditioned ray, no exception; one side's answer on the others
    assert np.array_equal(obj[well], j["ref_obj"][well]), np.nonzero(well & (obj != j["ref_obj"]))[0][:10]
    assert j["accepted"].all(), np.nonzero(~j["accepted"])[0][:10]
    # t, pos, normal of every hit (ill-conditioned ones against the side they chose)
    assert j["t_ok"][well].all(), np.nonzero(well & ~j["t_ok"])[0][:10]
    rows, col = np.arange(len(o)), np.maximum(j["col"], 0)                # a ray within the margin of parallel to the surface has no t to compare
    bt = np.array([b[R.KIND_NAMES[k]]["t"] for k in c["kind"][col]])
    notpar = c["cos"][rows, col] * c["ext"][rows, col] > R.MARGIN_FACTOR * bt * R.ulp32(c["ext"][rows, col])
    assert j["t_ok"][~well & notpar].all(), np.nonzero(~well & notpar & ~j["t_ok"])[0][:10]
    res = I.residual_ulp(kinds, params, obj, pos)
    kb = np.array([b[R.KIND_NAMES[kinds[max(i, 0)]]]["residual"] for i in obj])
    assert (res[well] <= kb[well]).all(), np.nonzero(well & (res > kb))[0][:10]
    assert SIDE_SHARE <= side <= 1 - SIDE_SHARE, side
    assert ill_random <= cap, ill_random


SETS = [(kind, i) for kind in range(4) for i in range(len(I.primitive_sets(kind))) if I.primitive_sets(kind)[i][5]]


@pytest.mark.parametrize("kind,i", SETS, ids=[R.KIND_NAMES[k] + "-" + I.primitive_sets(k)[i][0].replace(" ", "_") for k, i in SETS])
def test_primitive_against_binary64(oracle, kind, i):
    name, scene, o, d, aimed, _ = I.primitive_sets(kind)[i]
    osc = O.Scene.create(**scene)
    answer = I.oracle_casts(osc, o, d)
    check_intersections(R.KIND_NAMES[kind] + " / " + name, scene, o, d, aimed, answer, RANDOM_CAP)
    # Primitive::Intersect on its own gives the same bits as the scene's cast
    ob = O.OObject(kind, 0)
    for k, v in enumerate(scene["objects"][0][2]):
        ob.p[k] = v
    import ctypes as C
    t, pos, nrm = C.c_float(), (C.c_float * 3)(), (C.c_float * 3)()
    for r in range(0, len(o), 97):
        hit = oracle.oracle_intersect(C.byref(ob), O.f3(o[r]), O.f3(d[r]), C.byref(t), pos, nrm)
        assert bool(hit) == (answer[0][r] >= 0)
        if hit:
            assert np.float32(t.value).view(np.uint32) == answer[1][r].view(np.uint32) and np.array_equal(np.array(pos[:], np.float32), answer[2][r])


def test_mixed_scene_against_binary64(oracle):
    scene, o, d, aimed = I.mixed_set()
    osc = O.Scene.create(**scene)
    assert len(osc.objects()) == 106                                     # beyond the 80 objects at which AUTO leaves the two-phase engine
    check_intersections("mixed", scene, o, d, aimed, I.oracle_casts(osc, o, d), MIXED_CAP)


def test_sphere_takes_directions_as_unit(oracle):
    """Reference property, pinned: Sphere::Intersect solves its quadratic with a = 1 (primitive_sphere.cc:78), so for a direction that is
    not of unit length its t is a root of t^2 - 2 (c - o).d t + |c - o|^2 - r^2, not the distance to the geometric sphere in units of |d|."""
    for name, scene, o, d, aimed, geometric in I.primitive_sets(R.SPHERE):
        if geometric:
            continue
        osc = O.Scene.create(**scene)
        obj, t, pos, _ = I.oracle_casts(osc, o, d)
        roots, disc = R.sphere_roots_unit_a(np.array(scene["objects"][0][2] + [0] * 8)[:12], o, d)
        with np.errstate(all="ignore"):
            sure = np.abs(disc) > 1e-4 * np.maximum(1.0, np.abs(roots).max(1) ** 2)
            first = np.where(roots[:, 0] > 2 * R.KEPS, roots[:, 0], np.where(roots[:, 1] > 2 * R.KEPS, roots[:, 1], np.nan))
            clear = sure & ~((np.abs(roots - R.KEPS) < R.KEPS).any(1))
        hit = obj >= 0
        assert np.array_equal(hit[clear], np.isfinite(first)[clear])
        s = clear & hit
        assert s.sum() >= 10 and np.allclose(t[s], first[s], rtol=1e-3, atol=0)
        geo = R.candidates(R.SPHERE, np.array(scene["objects"][0][2] + [0] * 8)[:12], o, d)
        assert (np.abs(geo["t"][s] - t[s, None].astype(np.float64)).min(1) > 1e-2 * np.abs(t[s])).mean() > 0.9       # and it is not the geometric t


@pytest.mark.parametrize("name", [s[0] for s in I.MATERIAL_SETS])
def test_material_against_binary64(oracle, name):
    di, w, used = I.oracle_materials(name)
    check_materials(name, di, w, used)


def check_materials(name, di, w, used):
    kind, mats, importance, mat, nrm, do, state = I.material_items(name)
    ref = I.material_reference(name)
    b_dir, b_w, margin_items = I.material_bounds(BOUNDS["material"], name, mat)
    well = I.material_well(ref, margin_items)
    e_dir, e_w = I.material_errors(ref, di, w)
    print(f"{name}: {well.mean():.3f} well-conditioned, worst dir_in / weight error {e_dir[well].max():.2f} / {e_w[well].max():.2f} ulp")
    assert np.array_equal(used[well], ref["draws"][well])
    assert (e_dir[well] <= b_dir[well]).all() and (e_w[well] <= b_w[well]).all(), (np.nonzero(well & ((e_dir > b_dir) | (e_w > b_w)))[0][:10])
    # the others are classified: the answer of one side of every decision within the margin, draws included (a NaN is no such answer)
    assert np.isfinite(di).all() and np.isfinite(w).all()
    ok = I.material_classify(name, di, w, used, BOUNDS["material"])
    assert ok.all(), np.nonzero(~ok)[0][:10]
    bound = float(b_dir.max())
    tol = bound * 2.0 ** -23
    n64, do64, di64 = nrm.astype(np.float64), do.astype(np.float64), di.astype(np.float64)
    cos_o, cos_i = R.dot(do64, n64), R.dot(di64, n64)
    if kind == R.SPECULAR:                                               # the mirror direction: same tangential part reversed, same normal part
        assert np.abs(di64 + do64 - 2 * cos_o[:, None] * n64).max() <= tol
    if kind == R.LAMBERTIAN:
        assert (np.sign(cos_i[well]) == np.sign(cos_o[well])).all() and np.abs(R.norm(di64) - 1).max() <= 2 * tol
    if kind == R.REFRACTION:
        ior = np.array([I.MATERIALS[m][2] for m in mat], np.float32).astype(np.float64)
        margin = margin_items
        crit = slice(1400, 2000)                                         # the critical-angle items land on both sides, clearly and not
        assert 0.3 <= ref["tir"][crit].mean() <= 0.7
        sure_crit = (ref["cond_tir"] > margin)[crit]
        assert (sure_crit & ref["tir"][crit]).mean() >= 0.1 and (sure_crit & ~ref["tir"][crit]).mean() >= 0.1
        mirrored = np.abs(di64 + do64 - 2 * cos_o[:, None] * n64).max(1) <= 4 * tol
        sure_t = ref["cond_tir"] > margin
        assert (mirrored[sure_t & ref["tir"]]).all()                                                       # total internal reflection exactly where sin^2 beta > 1
        assert np.array_equal(used[sure_t] == 0, ref["tir"][sure_t])
        sure_c = sure_t & ~ref["tir"] & (ref["cond_choice"] > margin)
        assert np.array_equal(mirrored[sure_c], ref["reflect"][sure_c])                                    # the choice is u < p_r
        tr = sure_c & ~ref["reflect"]
        assert tr.sum() > 300
        sin_a, sin_b = R.norm(np.cross(do64, n64)), R.norm(np.cross(di64, n64))
        assert np.abs(sin_b[tr] - ref["ior"][tr] * sin_a[tr]).max() <= 8 * tol                             # Snell's law
        assert np.abs(R.dot(np.cross(do64, n64), di64))[tr].max() <= 8 * tol                               # coplanarity
        assert (np.sign(cos_i[tr]) == -np.sign(cos_o[tr])).all()                                           # to the other side
        scale2 = 1.0 if importance else ref["ior"] ** 2                                                    # the ior^2 factor: SampleLight only
        f0 = ((ior - 1) / (ior + 1)) ** 2
        rho_r = f0 + (1 - f0) * (1 - np.abs(cos_o)) ** 5
        rho_t = (1 - rho_r) * scale2
        p_r = ((rho_r / (rho_r + rho_t) if not importance else rho_r) + 0.5) / 2
        p_t = ((rho_t / (rho_r + rho_t) if not importance else rho_t) + 0.5) / 2
        expect = np.where(ref["reflect"], rho_r / p_r, rho_t / p_t)
        assert np.abs(w[sure_c, 0] - expect[sure_c]).max() <= bound * 2.0 ** -22


CAMS = [(cam, W, H) for cam in I.CAMERAS for W, H in I.FRAMES]


@pytest.mark.parametrize("cam,W,H", CAMS, ids=[f"{c}-{w}x{h}" for c, w, h in CAMS])
def test_eye_rays_land_in_their_pixel(oracle, cam, W, H):
    osc = O.Scene.create(**I.camera_scene(cam))
    check_eye(osc, cam, W, H, I.oracle_eye(osc, W, H))


def check_eye(osc, cam, W, H, eye):
    e = I.eye_reference(osc, cam, W, H, eye)
    b = BOUNDS["eye"][cam]
    print(f"{cam} {W}x{H}: worst overshoot of the pixel's rectangle {e['pixel'].max():.2f} ulp, off the blade {e['blade'].max():.2f} ulp, off the focus point {e['focus'].max():.2f} ulp")
    assert (e["pixel"] <= b["pixel"]).all(), (e["found"][e["pixel"] > b["pixel"]][:5], e["want"][e["pixel"] > b["pixel"]][:5])
    assert (e["blade"] <= b["blade"]).all()                              # the thin-lens origin lies on a blade
    assert (e["focus"] <= b["focus"]).all()                              # through the conjugate focus point of its pixel
    if "pinhole_origin" in e:
        assert (e["pinhole_origin"] == 0).all()                          # the pinhole origin is the lens origin exactly
    assert np.abs(R.norm(eye[:, 3:6].astype(np.float64)) - 1).max() < 4 * 2.0 ** -23

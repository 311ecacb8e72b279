"""The oracle against the binary64 statement of the same operations (tests/f64_reference.py) -- no GPU needed.

Bit parity proves that the kernels and the oracle are one function; these tests bound that function against the geometric and optical
definitions, on random inputs and on inputs aimed at the places where the answer changes (tests/f64_inputs.py).  Bounds: 4 x the
measured worst case of tests/golden/f64_reference_bounds.json; margins: 4 x the bounds.  A ray inside the margin of a boundary is
classified, not skipped: its answer must be one the binary64 reference gives on one side of that boundary.
The light side: the light table, the start of a light path, the lens response, and the camera generated and inverted (check_light, check_response, check_round_trip).
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


# ------------------------------------------------------------------------------------------------------------------
# light tracing: the light table, the start of a light path, the lens response
# ------------------------------------------------------------------------------------------------------------------
LIGHT_SETS = list(range(len(I.LIGHT_SET_NAMES)))
LIGHT_IDS = [name.replace(" / ", "-").replace(" ", "_") for name in I.LIGHT_SET_NAMES]


def check_light(name, scene, states, aimed, fam, got):
    """Shared with the GPU leg: `got` = (origin, dir, weight, scene index of the light, draws used) of some implementation for the states of one light set."""
    table, kinds, params = I.light_scene_table(scene)
    b = BOUNDS["light"]
    ref = R.light_ray(table, states)
    origin, direction, weight, obj, used = got
    margin = I.light_margin(b, table)
    well = ref["cond"] > margin
    e = I.light_errors(table, ref, origin, direction, weight)
    ib = I.light_item_bounds(b, table, ref)
    ill_random = float((~well[~aimed]).mean())
    print(f"{name}: {len(table['object'])} lights, ill-conditioned {ill_random:.4f} of the random half (cap {RANDOM_CAP}), {(~well[aimed]).mean():.3f} of the aimed half; worst "
          + " / ".join(f"{q} {e[q][well].max():.2f}" for q in I.LIGHT_QUANTITIES) + " ulp on well-conditioned items")
    assert np.isfinite(origin).all() and np.isfinite(direction).all() and np.isfinite(weight).all()
    # the light and the number of draws: the binary64 answer on every well-conditioned item, no exception
    assert np.array_equal(obj[well], ref["object"][well]), np.nonzero(well & (obj != ref["object"]))[0][:10]
    assert np.array_equal(used[well], ref["draws"][well])
    if len(table["object"]) == 2 and table["power"][0] == table["power"][1]:
        on = ref["u"][:, 0] == 0.5                                        # two equal powers: u x total is the first running sum without a rounding, in either
        assert on.sum() >= 10 and (obj[on] == table["object"][0]).all()   # arithmetic: "the first cumulative power >= u x total" is decided exactly
    for q in I.LIGHT_QUANTITIES:
        assert (e[q][well] <= ib[q][well]).all(), (q, np.nonzero(well & (e[q] > ib[q]))[0][:10])
    d64 = direction.astype(np.float64)
    assert np.abs(R.norm(d64) - 1).max() <= 4 * 2.0 ** -23
    assert (R.dot(d64, R.unit(ref["normal"]))[well] >= -ib["dir"][well] * 2.0 ** -23).all()                 # into the hemisphere of the surface normal
    tri = well & (table["kind"][ref["light"]] == R.TRIANGLE)
    if tri.any():                                                        # a triangle's points lie inside it: signed distance from every edge line
        p = table["params"][ref["light"][tri]]
        A, B, Cc = p[:, :3], p[:, 3:6], p[:, 6:9]
        nh = R.unit(np.cross(B - A, Cc - A))
        P = origin[tri].astype(np.float64)
        inside = np.min([R.dot(np.cross(Vb - Va, P - Va), nh) / R.norm(Vb - Va) for Va, Vb in ((A, B), (B, Cc), (Cc, A))], 0)
        assert (inside >= -ib["origin"][tri] * R.ulp32(I.light_scale(table, ref, origin)[tri])).all()
    # every other item is classified: the binary64 answer on one side of the decisions within the margin
    ok = I.light_classify(table, states, got, b)
    assert ok.all(), np.nonzero(~ok)[0][:10]
    side = I.light_side(fam, ref, table)
    for f, label in I.LIGHT_FAMILIES.items():
        if (fam == f).any():
            share = float(side[fam == f].mean())
            print(f"  aimed at {label}: {int((fam == f).sum())} items, {share:.3f} on the far side")
            assert SIDE_SHARE <= share <= 1 - SIDE_SHARE, (label, share)
    assert ill_random <= RANDOM_CAP, ill_random


def check_light_table(scene, olights, flat=None):
    """The oracle's light set (and, `flat`, the host model's: equal bits) against f64_reference.light_table.  Tolerances from the operations:
    a power is an area (at most 9 roundings for a triangle's cross product, length and half) times pi rho summed over three channels (7
    more): 16 half-ulp = 8 ulp; every running sum adds one rounding of a value no larger than itself: 8 + k / 2 ulp for entry k.
    irradiance = rho x binary32 pi: 1 ulp.  pdf_area = sum(irradiance) / total: 3 ulp for the sum, the total's own bound, the division."""
    table = I.light_scene_table(scene)[0]
    obj, cum, irr = olights
    n = len(obj)
    assert np.array_equal(obj, table["object"])
    k = np.arange(n)
    assert (np.abs(cum - table["cum_power"]) <= (8 + k / 2) * R.ulp32(table["cum_power"])).all()
    assert (np.abs(irr - table["irradiance"]) <= R.ulp32(table["irradiance"])).all()
    if n > 1:
        assert (np.diff(cum.astype(np.float64)) >= 0).all()
    if flat is not None:
        assert len(flat) == n
        assert np.array_equal(np.array([f.object for f in flat], np.uint32), obj)
        assert np.array_equal(np.array([f.cum_power for f in flat], np.float32).view(np.uint32), cum.view(np.uint32))
        assert np.array_equal(np.array([f.irradiance[:] for f in flat], np.float32).reshape(n, 3).view(np.uint32), irr.view(np.uint32))
        pdf = np.array([f.pdf_area for f in flat], np.float32)
        assert np.array_equal(pdf.view(np.uint32), (((irr[:, 0] + irr[:, 1]) + irr[:, 2]) / cum[-1]).view(np.uint32))     # light_set.h:107-111 in binary32
        assert (np.abs(pdf - table["pdf_area"]) <= (4 + 8 + n / 2) * R.ulp32(table["pdf_area"])).all()
    return table


@pytest.mark.parametrize("i", LIGHT_SETS, ids=LIGHT_IDS)
def test_light_ray_against_binary64(oracle, i):
    name, scene, states, aimed, fam = I.light_sets()[i]
    check_light(name, scene, states, aimed, fam, I.oracle_light(O.Scene.create(**scene), states))


@pytest.mark.parametrize("i", LIGHT_SETS, ids=LIGHT_IDS)
def test_light_table_against_binary64(amber, oracle, i):
    name, scene, *_ = I.light_sets()[i]
    hs = amber.HostScene.create(**scene)
    table = check_light_table(scene, O.Scene.create(**scene).lights(), hs.lights())
    hs.close()
    if name == "mixed / 40":
        assert table["power"][-1] / table["power"][0] >= 1e6 and (np.diff(table["power"]) > 0).all()      # six decades, all distinct
    if name in ("mixed / 2", "mixed / 5"):
        assert (np.diff(table["power"]) == 0).sum() == 1 and len(table["object"]) <= 16                    # one pair of exactly equal powers, in scene order
        k = int(np.nonzero(np.diff(table["power"]) == 0)[0][0])
        assert table["object"][k] < table["object"][k + 1]


def test_a_scene_without_lights_has_no_light_rays(oracle):
    osc = O.Scene.create(**I.camera_scene("thin6"))
    assert len(osc.lights()[0]) == 0
    with pytest.raises(ValueError, match="no lights"):
        osc.light_rays(np.ones(4, np.uint64))


def test_sphere_lights_emit_from_one_hemisphere_only(oracle):
    """Reference property, pinned: Sphere::SampleSurfacePoint takes SphereSA's (r0 cos phi, r0 sin phi, sqrt(1 - r0^2)) with r0 uniform in
    [-1, 1) (primitive_sphere.cc:115-122, sampling.h:185-199) as the point's direction from the centre.  That is no uniform sphere: its z is
    never negative, and z = sqrt(1 - r0^2) piles up near 1 (half of the points have z > sqrt(3) / 2 = 0.866; a uniform hemisphere has 13 %
    there).  The project reproduces it; a "fix" on either side has to show here."""
    name, scene, states, aimed, fam = next(s for s in I.light_sets() if s[0] == "sphere / base")
    table = I.light_scene_table(scene)[0]
    o, d, w, obj, used = I.oracle_light(O.Scene.create(**scene), states[~aimed])
    pos = {int(ob): k for k, ob in enumerate(table["object"])}
    p = table["params"][[pos[int(ob)] for ob in obj]]
    local = (o.astype(np.float64) - p[:, :3]) / p[:, 3:4]
    assert (local[:, 2] >= 0).all()
    assert np.abs(R.norm(local) - 1).max() < 1e-5
    assert 0.45 <= (local[:, 2] > np.sqrt(3) / 2).mean() <= 0.55


def response_side(ref, boundary):
    axis, value = boundary
    return np.where(axis == 2, ref["z"] >= 0, np.where(axis == 0, ref["pixel"][:, 0] >= value, ref["pixel"][:, 1] >= value))


def check_response(osc, cam, W, H, got):
    """Shared with the GPU leg: `got` = (reached, pixel index, value) of some implementation for the rays of response_items(cam, W, H)."""
    pos, do, aimed, fam, boundary, outside = I.response_items(cam, W, H)
    thin = I.CAMERAS[cam]["n_blades"] > 0
    b = BOUNDS["response"][cam]
    ref = I.response_reference(osc, cam, W, H, pos, do)
    reached, pixel, value = got
    e = I.response_errors(ref, W, H, reached, pixel, value, thin)
    well = I.response_well(ref, W, H, b, thin) & ~outside
    ill_random = float((~well[~aimed]).mean())
    print(f"{cam} {W}x{H}: ill-conditioned {ill_random:.4f} of the random half (cap {RANDOM_CAP}), {(~well[aimed]).mean():.3f} of the aimed half; reached {ref['reached'][~aimed].mean():.3f} of the "
          f"random and {ref['reached'][aimed].mean():.3f} of the aimed half; image point at most {e['over'][~outside].max():.2f} ulp from the answer, value within {e['value'][well].max():.2f} ulp; "
          f"{int(outside.sum())} items outside the contract (pinhole, local z = 0)")
    # outside the contract: either no response, or a pixel of the frame and a finite value
    assert ((reached[outside] == 0) | (pixel[outside] < W * H)).all() and np.isfinite(value[outside]).all()
    assert outside.sum() == (RESPONSE_OUTSIDE if not thin else 0)
    r = reached.astype(bool)
    assert (pixel[r] < W * H).all() and (pixel[~r] == 0).all() and (value[~r] == 0).all() and np.isfinite(value).all()
    # well-conditioned: the binary64 decision and the floor of the binary64 pixel, no exception
    assert np.array_equal(r[well], ref["reached"][well]), np.nonzero(well & (r != ref["reached"]))[0][:10]
    assert np.array_equal(pixel[well & r], ref["index"][well & r])
    assert (e["value"][well] <= b["value"]).all()
    # the others: the answer of one side of the boundary within the margin (the neighbouring pixel, reached or not)
    keep = ~outside
    assert (e["over"][keep] <= R.MARGIN_FACTOR * b["pixel"]).all(), np.nonzero(keep & (e["over"] > R.MARGIN_FACTOR * b["pixel"]))[0][:10]
    both = keep & r & ref["reached"]
    assert (e["value"][both] <= b["value"]).all()                        # the value has no discontinuity on the sensor
    side = response_side(ref, boundary)
    for g, label in I.RESPONSE_FAMILIES.items():
        s = (fam == g) & keep
        share = float(side[s].mean())
        print(f"  aimed at {label}: {int(s.sum())} items, {share:.3f} on the far side")
        assert SIDE_SHARE <= share <= 1 - SIDE_SHARE, (label, share)
    assert ill_random <= RANDOM_CAP, ill_random


RESPONSE_OUTSIDE = 19        # of response_items' aimed half: every sixth item is of the local-z family, every ninth of those has step 0


@pytest.mark.parametrize("cam,W,H", CAMS, ids=[f"{c}-{w}x{h}" for c, w, h in CAMS])
def test_lens_response_against_binary64(oracle, cam, W, H):
    osc = O.Scene.create(**I.camera_scene(cam))
    pos, do, *_ = I.response_items(cam, W, H)
    check_response(osc, cam, W, H, osc.lens_responses(W, H, pos, do, math=O.MATH_GLIBC))


def check_round_trip(osc, cam, W, H, eye, got):
    """The camera generated one way and inverted the other: `got` = the lens response (reached, pixel, value) of the eye rays `eye` of frame W x H."""
    thin = I.CAMERAS[cam]["n_blades"] > 0
    b = BOUNDS["response"][cam]
    reached, pixel, value = got
    px, _ = I.eye_items(W, H)
    assert (reached == 1).all()
    ref, k = I.eye_weight_reference(osc, cam, W, H, eye)
    margin = R.MARGIN_FACTOR * b["pixel"] * R.ulp32(max(W, H))
    own = pixel == px
    moved = ~own                                                          # only across a pixel edge the ray lies within the margin of, to the neighbour there
    dx, dy = pixel.astype(np.int64) % W - px.astype(np.int64) % W, pixel.astype(np.int64) // W - px.astype(np.int64) // W
    assert (np.abs(dx[moved]) + np.abs(dy[moved]) >= 1).all() and (np.maximum(np.abs(dx), np.abs(dy))[moved] == 1).all()
    assert (ref["edge"][moved] <= margin).all()
    over = I.response_errors(ref, W, H, reached, pixel, value, thin)["over"]
    assert (over <= R.MARGIN_FACTOR * b["pixel"]).all()
    print(f"{cam} {W}x{H}: {int(moved.sum())} of {len(px)} eye rays come back in a neighbouring pixel")
    if thin:
        err = np.abs(value.astype(np.float64) * k - eye[:, 6]) / R.ulp32(eye[:, 6])
        print(f"  value x 1 / p_area / pdf_dir against the eye ray's weight: at most {err.max():.2f} ulp (bounds {b['value']:.1f} + {b['eye_weight']:.1f})")
        assert (err <= b["value"] + b["eye_weight"]).all()
    else:
        assert (value == 1).all()


@pytest.mark.parametrize("cam,W,H", CAMS, ids=[f"{c}-{w}x{h}" for c, w, h in CAMS])
def test_eye_rays_come_back_through_the_lens_oracle(oracle, cam, W, H):
    osc = O.Scene.create(**I.camera_scene(cam))
    eye = I.oracle_eye(osc, W, H)
    check_round_trip(osc, cam, W, H, eye, osc.lens_responses(W, H, eye[:, :3], eye[:, 3:6], math=O.MATH_GLIBC))

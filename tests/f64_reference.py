"""The path's primitives, materials, eye rays, light table, light rays and lens response once more, in binary64 numpy, from their geometric and optical definitions.

The oracle and the kernels are the same function by construction (bit parity); this module is a third statement that shares
no order of operations with either.  It imports numpy only.  Inputs are binary32 values widened exactly.  Every function
returns the mathematically defined answer AND how far the input is from the nearest point where that answer changes
discontinuously (its conditioning), so that a comparison can tell a wrong kernel from an input on which binary32 cannot decide.

Conventions
  * t is in units of |dir|; a hit needs t > kEPS = 1e-6.
  * All conditioning measures are distances in scene units.  A binary32 hit point is displaced by a few ulp NORMAL to the
    surface; along the surface it slides by that amount / |cos| of the angle of incidence.  So every error of t, pos and normal is
    taken times |cos| (the displacement normal to the surface), and every in-surface conditioning measure (distance to a
    triangle's edge, a disk's rim, a cylinder's end; t - kEPS) is taken times |cos| too.  A ray parallel to a surface
    (|det| or |cos| -> 0, a -> 0 for the cylinder) has conditioning 0: its t is not defined.  That measure is relative (|cos| against
    a few ulp of 1), so it is expressed at the scale the ray's ulp is taken at: |cos| x max(|o|, |t d|, extent).
  * The cylinder is open, axis from `center` along `normal`, 0 <= h <= height.  The disk's normal is used as given.
  * Normals: triangle Normalize(E1 x E2); sphere and cylinder the outward unit normal at the hit; disk `normal` as given.
    None is flipped towards the ray.

`python tests/f64_reference.py --measure` compares the ORACLE with this module on the inputs of tests/f64_inputs.py and writes
tests/golden/f64_reference_bounds.json (the worst error per quantity, in ulp); the tests take 4x those as bounds and 4x the
bounds as the ill-conditioning margin.
"""
import numpy as np

KEPS = 1e-6
TRIANGLE, SPHERE, DISK, CYLINDER = 0, 1, 2, 3
LAMBERTIAN, PHONG, SPECULAR, REFRACTION, DIFFUSE_LIGHT, EYE = 0, 1, 2, 3, 4, 5
KIND_NAMES = ("triangle", "sphere", "disk", "cylinder")
PHONG_MAX_TRIES = 1024
BOUND_FACTOR, MARGIN_FACTOR = 4.0, 4.0          # bound = 4 x measured worst case; margin = 4 x bound


def dot(a, b):
    return np.einsum("...i,...i->...", a, b)


def norm(a):
    return np.sqrt(dot(a, a))


def unit(a):
    return a / norm(a)[..., None]


def ulp32(x):
    """The spacing of binary32 numbers at magnitude x."""
    x = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(x)) - 23)


def _smin(*ms):
    out = ms[0]
    for m in ms[1:]:
        out = np.minimum(out, m)
    return out


def extent(kind, p):
    """Largest coordinate magnitude the primitive reaches: the natural scale of its binary32 arithmetic."""
    p = np.asarray(p, np.float64)
    if kind == TRIANGLE:
        return float(np.abs(p[:9]).max())
    if kind == SPHERE:
        return float(np.abs(p[:3]).max() + p[3])
    return float(np.abs(p[:3]).max() + p[6] + (p[7] if kind == CYLINDER else 0.0))


# ------------------------------------------------------------------------------------------------------------------
# one primitive: the candidate roots of a ray, each with its signed validity margin
# ------------------------------------------------------------------------------------------------------------------
def candidates(kind, p, o, d):
    """The (up to two) points where the line o + t d meets the primitive's unbounded surface, nearest first.
    Returns t (n, 2), m (n, 2), pos (n, 2, 3), normal (n, 2, 3), cos (n, 2), resid(point) -> distance from the surface.
    m > 0: the candidate is a hit, and stays one under any displacement below m; m < 0: it is none by |m|."""
    p = np.asarray(p, np.float64)
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    n = len(o)
    ld = norm(d)
    dh = d / ld[:, None]
    ext = extent(kind, p)
    t = np.full((n, 2), np.inf)
    m = np.full((n, 2), -np.inf)
    pos = np.zeros((n, 2, 3))
    nrm = np.zeros((n, 2, 3))
    cos = np.zeros((n, 2))
    with np.errstate(all="ignore"):
        if kind in (TRIANGLE, DISK):
            A = p[:3]
            if kind == TRIANGLE:
                B, Cc = p[3:6], p[6:9]
                N = np.cross(B - A, Cc - A)
                if norm(N) == 0:                                 # a degenerate triangle (the pinhole's aperture) is no surface: never a candidate
                    return dict(t=t, m=m, pos=pos, normal=nrm, cos=cos, ext=np.full((n, 2), ext), ld=ld)
                normal = N / norm(N)
            else:
                N = p[3:6]
                normal = N
            nh = N / norm(N)
            c = np.abs(dot(dh, nh))
            tt = dot(A - o, nh) / dot(d, nh)
            P = o + tt[:, None] * d
            if kind == TRIANGLE:
                inside = np.inf
                for Va, Vb in ((A, B), (B, Cc), (Cc, A)):
                    e = Vb - Va
                    inside = np.minimum(inside, dot(np.cross(e, P - Va), nh) / norm(e))       # signed distance to the edge line, + inside
            else:
                inside = p[6] - norm(P - A)                                                   # distance to the rim, + inside
            mm = _smin(inside * c, (tt - KEPS) * ld * c)
            big = np.maximum(np.maximum(np.abs(o).max(1), np.abs(tt) * np.abs(d).max(1)), ext)
            big = np.where(np.isfinite(big), big, ext)
            mm = np.sign(mm) * np.minimum(np.abs(mm), big * c)                                # |det| / |cos| against 0: relative, so at the scale its ulp is taken at
            ok = np.isfinite(tt)
            t[:, 0] = np.where(ok, tt, np.inf)
            m[:, 0] = np.where(ok, mm, -0.0)
            pos[:, 0] = np.where(ok[:, None], P, 0.0)
            nrm[:, 0] = normal
            cos[:, 0] = c
        else:
            A = p[:3]
            if kind == SPHERE:
                r = p[3]
                w = o - A
                dp = ld
                dph = dh
                wp = w
            else:
                nh = p[3:6] / norm(p[3:6])
                r, H = p[6], p[7]
                w = o - A
                dperp = d - dot(d, nh)[:, None] * nh
                dp = norm(dperp)
                dph = dperp / dp[:, None]
                wp = w - dot(w, nh)[:, None] * nh
            sc = -dot(wp, dph)                                   # distance along the (projected) ray to the point nearest the centre / axis
            rho = norm(wp + sc[:, None] * dph)                   # distance of the line from the centre / axis
            g = r - rho                                          # the discriminant against 0, in scene units
            half = np.sqrt(np.maximum(r * r - rho * rho, 0.0))
            for k, sgn in enumerate((-1.0, 1.0)):
                s = sc + sgn * half
                tk = s / dp
                P = o + tk[:, None] * d
                c = (dp / ld) * half / r                         # |cos| of the angle of incidence
                mk = _smin(g, (tk - KEPS) * ld * c)
                if kind == SPHERE:
                    nk = (P - A) / r
                else:
                    h = dot(P - A, nh)
                    mk = _smin(mk, h * c, (H - h) * c)
                    nk = (P - A - h[:, None] * nh) / r
                    big = np.maximum(np.maximum(np.abs(o).max(1), np.abs(tk) * np.abs(d).max(1)), ext)
                    mk = np.sign(mk) * np.minimum(np.abs(mk), np.where(np.isfinite(big), big, ext) * dp / ld)
                ok = np.isfinite(tk)
                t[:, k] = np.where(ok, tk, np.inf)
                m[:, k] = np.where(ok, mk, -0.0)
                pos[:, k] = np.where(ok[:, None], P, 0.0)
                nrm[:, k] = np.where(ok[:, None], nk, 0.0)
                cos[:, k] = np.where(ok, c, 0.0)
    return dict(t=t, m=m, pos=pos, normal=nrm, cos=cos, ext=np.full((n, 2), ext), ld=ld)


def sphere_roots_unit_a(p, o, d):
    """The roots of t^2 - 2 (c - o).d t + |c - o|^2 - r^2: the sphere's quadratic with a = 1, i.e. with |d| taken as 1 whatever it is.
    Returns (roots (n, 2) ascending, NaN without real roots; discriminant)."""
    p, o, d = np.asarray(p, np.float64), np.asarray(o, np.float64), np.asarray(d, np.float64)
    co = p[:3] - o
    b, c = -2.0 * dot(co, d), dot(co, co) - p[3] * p[3]
    disc = b * b - 4.0 * c
    with np.errstate(all="ignore"):
        s = np.sqrt(disc)
    return np.stack([(-b - s) / 2.0, (-b + s) / 2.0], 1), disc


def residual(kind, p, pts):
    """Distance of pts from the primitive's unbounded surface (its implicit equation, in scene units)."""
    p, pts = np.asarray(p, np.float64), np.asarray(pts, np.float64)
    A = p[:3]
    if kind == TRIANGLE:
        N = np.cross(p[3:6] - A, p[6:9] - A)
        return np.abs(dot(pts - A, N / norm(N)))
    if kind == DISK:
        return np.abs(dot(pts - A, p[3:6] / norm(p[3:6])))
    if kind == SPHERE:
        return np.abs(norm(pts - A) - p[3])
    nh = p[3:6] / norm(p[3:6])
    w = pts - A
    return np.abs(norm(w - dot(w, nh)[:, None] * nh) - p[6])


def scene_candidates(kinds, params, o, d):
    """Candidates of every object of a scene, side by side: arrays (n, 2 * n_objects) and `obj`, the object of every column."""
    parts = [candidates(int(k), p, o, d) for k, p in zip(kinds, params)]
    out = {key: np.concatenate([c[key] for c in parts], 1) for key in ("t", "m", "pos", "normal", "cos", "ext")}
    out["ld"] = parts[0]["ld"]
    out["obj"] = np.repeat(np.arange(len(parts)), 2)
    out["kind"] = np.repeat(np.asarray(kinds, np.int64), 2)
    return out


def closest(c):
    """The binary64 answer: the smallest root with t > kEPS over all candidates, the lower object index on a tie.
    Returns (object or -1, column or -1, gap): gap = distance along the ray to the second-nearest valid candidate of ANOTHER object."""
    t = np.where(c["m"] > 0, c["t"], np.inf)
    col = np.argmin(t, 1)                                        # first minimum: the lower index on a tie
    rows = np.arange(len(t))
    hit = np.isfinite(t[rows, col])
    obj = np.where(hit, c["obj"][col], -1)
    other = np.where(c["obj"][None, :] != obj[:, None], t, np.inf)
    gap = (other.min(1) - t[rows, col]) * c["ld"]
    return obj, np.where(hit, col, -1), np.where(hit, gap, np.inf)


def judge(c, got_obj, got_t, got_pos, got_normal, bounds, o, d):
    """Compares an implementation's closest hits with the binary64 candidates.
    bounds: {kind name: {"t", "pos", "normal": ulp}} -- the error bounds in force (already 4 x the measured worst case).
    Returns a dict of per-ray arrays:
      well       no candidate is within the margin of changing its validity and no other object's hit is within the margin of the nearest
      accepted   the answer is one the binary64 reference gives on one side of every boundary within the margin
                 (for a well-conditioned ray that is exactly the binary64 answer)
      col        the candidate the answer was matched with (-1: miss)
      err_t, err_pos, err_normal   errors against that candidate, in ulp of max(|o|, |t d|, extent), normal to the surface
      t_ok       err_* within bounds"""
    n = len(c["t"])
    rows = np.arange(n)
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    got_t = np.asarray(got_t, np.float64)
    with np.errstate(all="ignore"):
        scale = np.maximum(np.maximum(np.abs(o).max(1)[:, None], np.abs(c["t"] * np.abs(d).max(1)[:, None])), c["ext"])
        scale = np.where(np.isfinite(scale), scale, c["ext"])
        u = ulp32(scale)
        bt = np.array([bounds[KIND_NAMES[k]]["t"] for k in c["kind"]])[None, :] * u          # absolute bound, normal to the surface
        margin = MARGIN_FACTOR * bt
        sure = c["m"] > margin
        unsure = np.abs(c["m"]) <= margin
        slack = margin / np.maximum(c["cos"], 1e-300)                                        # the same along the ray
        obj, col, gap = closest(c)
        nom_slack = np.where(col >= 0, slack[rows, np.maximum(col, 0)], 0.0)
        tnom = np.where(col >= 0, c["t"][rows, np.maximum(col, 0)], np.inf)
        near = (c["m"] > 0) & (c["obj"][None, :] != obj[:, None]) & ((c["t"] - tnom[:, None]) * c["ld"][:, None] <= slack + nom_slack[:, None])
        relevant = (c["t"] - tnom[:, None]) * c["ld"][:, None] <= slack + nom_slack[:, None]   # a candidate behind the nearest hit cannot change the answer
        well = ~(unsure & relevant).any(1) & ~near.any(1)
        # match the answer with a candidate of its object
        hit = np.asarray(got_obj) >= 0
        mine = c["obj"][None, :] == np.asarray(got_obj)[:, None]
        et = np.where(mine, np.abs(got_t[:, None] - c["t"]) * c["ld"][:, None] * c["cos"], np.inf)
        et = np.where(np.isnan(et), np.inf, et)
        k = np.argmin(np.where(mine & ~(c["m"] < -margin), et, np.inf), 1)                   # nearest candidate that is not certainly invalid
        k = np.where(np.isfinite(np.where(mine & ~(c["m"] < -margin), et, np.inf)[rows, k]), k, np.argmin(et, 1))
        ck = lambda a: a[rows, k]
        tk, cosk, uk = ck(c["t"]), ck(c["cos"]), ck(u)
        err_t = np.where(hit, np.abs(got_t - tk) * c["ld"] * cosk / uk, 0.0)
        err_pos = np.where(hit, np.abs(np.asarray(got_pos, np.float64) - c["pos"][rows, k]).max(1) * cosk / uk, 0.0)
        nref = c["normal"][rows, k]
        kk = c["kind"][k]
        curved = np.isin(kk, (SPHERE, CYLINDER))
        dn = np.abs(np.asarray(got_normal, np.float64) - nref).max(1)
        radius = ck(c["radius"]) if "radius" in c else 1.0
        err_n = np.where(hit, np.where(curved, dn * radius * cosk / uk, dn / ulp32(np.abs(nref).max(1))), 0.0)
        kb = lambda q: np.array([bounds[KIND_NAMES[x]][q] for x in kk])
        t_ok = ~hit | ((err_t <= kb("t")) & (err_pos <= kb("pos")) & (err_n <= kb("normal")))
        # accepted: the matched candidate is not certainly invalid, and no certainly valid candidate lies certainly in front of it
        front = sure & ((tk[:, None] - c["t"]) * c["ld"][:, None] > slack + ck(slack)[:, None])
        front[rows, k] = False
        acc_hit = ~(ck(c["m"]) < -ck(margin)) & ~front.any(1)
        accepted = np.where(hit, acc_hit, ~sure.any(1))
    return dict(well=well, accepted=accepted, col=np.where(hit, k, -1), err_t=err_t, err_pos=err_pos, err_normal=err_n, t_ok=t_ok,
                ref_obj=obj, ref_col=col)


def with_radius(c, kinds, params):
    """Adds the column `radius` (curved primitives: the normal's error is the hit point's error / radius)."""
    r = [p[3] if k == SPHERE else (p[6] if k == CYLINDER else 1.0) for k, p in zip(kinds, np.asarray(params, np.float64))]
    c["radius"] = np.broadcast_to(np.repeat(np.array(r), 2)[None, :], c["t"].shape)
    return c


# ------------------------------------------------------------------------------------------------------------------
# materials
# ------------------------------------------------------------------------------------------------------------------
def xorshift_uniform(state):
    """One step of the sampler: xorshift64 (13, 7, 17), uniform = top 24 bits x 2^-24.  state: uint64 array, updated in place."""
    state ^= state << np.uint64(13)
    state ^= state >> np.uint64(7)
    state ^= state << np.uint64(17)
    return (state >> np.uint64(40)).astype(np.float64) * 2.0 ** -24


def _frame(w, flip=False):
    """The tangent frame the samplers use: u = w x e normalised, e the x axis where |w.x| < |w.y| and the y axis otherwise; v = w x u normalised."""
    e = np.where(((np.abs(w[:, 0]) < np.abs(w[:, 1])) != flip)[:, None], np.array([1.0, 0, 0]), np.array([0, 1.0, 0]))
    u = unit(np.cross(w, e))
    return u, unit(np.cross(w, u))


def _lobe(w, cos_t, r1, flip=False):
    u, v = _frame(w, flip)
    sin_t = np.sqrt(np.maximum(1.0 - cos_t * cos_t, 0.0))
    phi = 2.0 * np.pi * r1
    return u * (sin_t * np.cos(phi))[:, None] + v * (sin_t * np.sin(phi))[:, None] + w * cos_t[:, None]


def sample_material(kind, rho, param, normal, dir_out, state, importance=False, side=(0.0, 0.0, 0.0, False), follow=None):
    """dir_in, weight and the number of draws of one material kind for n items (normal, dir_out: (n, 3); state: (n,) uint64).
    cond: the distance of the item from a discontinuity of the answer (a sign decision, the total-reflection threshold, u against p_r,
    a Phong rejection, the choice of frame axis).  Refraction also returns tir, reflect, p_r, u, sin2_beta, ior (the ratio in use).

    side = (b_sign, b_threshold, b_choice, other_axis): the answer on one side of the decisions -- every sign decision on dir_out . n is taken
    as if the product were larger by b_sign, the total-reflection test as if sin^2 beta were larger by b_threshold, u < p_r (and a Phong
    rejection) as if the left side were smaller by b_choice, and the frame axis is the other one.  (0, 0, 0, False) is the binary64 answer.
    follow (Phong): accept at attempt follow[i] instead; `follow_valid` then says whether that is an answer of the rejection loop when every
    decision within |b_choice| may go either way (earlier attempts rejectable, this one acceptable)."""
    b_sign, b_thr, b_choice, other_axis = side
    nrm, do = np.asarray(normal, np.float64), np.asarray(dir_out, np.float64)
    rho = np.asarray(rho, np.float64)
    n = len(nrm)
    st = np.array(state, np.uint64).copy()
    draws = np.zeros(n, np.int64)
    cos_o = dot(do, nrm)
    mirror = 2.0 * cos_o[:, None] * nrm - do
    out = {}
    with np.errstate(all="ignore"):
        if kind == LAMBERTIAN:
            w = np.where((cos_o + b_sign > 0)[:, None], nrm, -nrm)
            r0, r1 = xorshift_uniform(st), xorshift_uniform(st)
            draws += 2
            di = _lobe(w, np.sqrt(r0), r1, other_axis)
            weight = np.broadcast_to(rho, (n, 3)).copy()
            cond = np.minimum(np.abs(cos_o), np.abs(np.abs(w[:, 0]) - np.abs(w[:, 1])))
        elif kind == PHONG:
            di = np.zeros((n, 3))
            cos_i = np.zeros(n)
            cond = np.abs(np.abs(mirror[:, 0]) - np.abs(mirror[:, 1]))
            todo = np.ones(n, bool)
            valid = np.ones(n, bool)
            for attempt in range(1, PHONG_MAX_TRIES + 1):
                idx = np.nonzero(todo)[0]
                if len(idx) == 0:
                    break
                s = st[idx]
                r0, r1 = xorshift_uniform(s), xorshift_uniform(s)
                st[idx] = s
                draws[idx] += 2
                cand = _lobe(mirror[idx], np.power(r0, 1.0 / (param + 1.0)), r1, other_axis)
                ci = dot(cand, nrm[idx])
                cond[idx] = np.minimum(cond[idx], np.abs(ci * cos_o[idx]))
                take = ~(cos_o[idx] * ci + b_choice <= 0) | (attempt == PHONG_MAX_TRIES)
                if follow is not None:
                    take = np.asarray(follow)[idx] == attempt
                    prod = cos_o[idx] * ci
                    valid[idx] &= np.where(take, (prod > -abs(b_choice)) | (attempt == PHONG_MAX_TRIES), prod <= abs(b_choice))
                    take |= attempt == PHONG_MAX_TRIES
                di[idx[take]], cos_i[idx[take]] = cand[take], ci[take]
                todo[idx[take]] = False
            weight = ((param + 2.0) / (param + 1.0) * np.abs(cos_i))[:, None] * rho
            out.update(follow_valid=valid)
        elif kind == SPECULAR:
            di, weight, cond = mirror, np.broadcast_to(rho, (n, 3)).copy(), np.full(n, np.inf)
        elif kind == REFRACTION:
            ior = np.where(cos_o + b_sign > 0, 1.0 / param, param)                      # the ratio n_from / n_to for light arriving along -dir_out
            sin2_b = (1.0 - cos_o * cos_o) * ior * ior                        # Snell: sin(beta) = ratio x sin(alpha)
            tir = sin2_b + b_thr > 1.0
            cos_b = np.sqrt(np.maximum(1.0 - sin2_b, 0.0))
            tangential = do - cos_o[:, None] * nrm
            dir_t = -ior[:, None] * tangential - (np.where(cos_o + b_sign > 0, 1.0, -1.0) * cos_b)[:, None] * nrm
            f0 = ((param - 1.0) / (param + 1.0)) ** 2
            rho_r = f0 + (1.0 - f0) * (1.0 - np.abs(cos_o)) ** 5              # Schlick
            if importance:
                rho_t = 1.0 - rho_r
                p_r, p_t = (rho_r + 0.5) / 2.0, (rho_t + 0.5) / 2.0
            else:
                rho_t = (1.0 - rho_r) * ior * ior                             # radiance is scaled by the squared ratio
                p_r, p_t = (rho_r / (rho_r + rho_t) + 0.5) / 2.0, (rho_t / (rho_r + rho_t) + 0.5) / 2.0
            s = st[~tir]
            u = np.full(n, np.nan)
            u[~tir] = xorshift_uniform(s)
            st[~tir] = s
            draws[~tir] += 1
            reflect = tir | (u - b_choice < p_r)
            di = np.where(reflect[:, None], mirror, dir_t)
            w1 = np.where(tir, 1.0, np.where(reflect, rho_r / p_r, rho_t / p_t))
            weight = w1[:, None] * rho
            cond = _smin(np.abs(cos_o), np.abs(1.0 - sin2_b), np.where(tir, np.inf, np.abs(u - p_r)))
            out.update(tir=tir, reflect=reflect, p_r=p_r, p_t=p_t, rho_r=rho_r, rho_t=rho_t, u=u, sin2_beta=sin2_b, ior=ior, dir_t=dir_t,
                       cond_tir=np.minimum(np.abs(cos_o), np.abs(1.0 - sin2_b)), cond_choice=np.where(tir, np.inf, np.abs(u - p_r)))
        elif kind == EYE:
            di, weight, cond = -do, np.ones((n, 3)), np.full(n, np.inf)
        else:
            di, weight, cond = np.zeros((n, 3)), np.zeros((n, 3)), np.full(n, np.inf)
    out.update(dir_in=di, weight=weight, draws=draws, state=st, cond=cond, mirror=mirror, cos_o=cos_o)
    return out


# ------------------------------------------------------------------------------------------------------------------
# eye ray -> pixel
# ------------------------------------------------------------------------------------------------------------------
def eye_ray_to_pixel(lens_kind, lens_origin, rotation, focus_distance, sensor_distance, blades, width, height, sensor_w, sensor_h, origin, direction):
    """Inverts the camera: which sensor point does the ray (origin, direction) image?
    lens_kind 0: thin lens (the ray leaves the aperture and passes the point of the focus plane that is conjugate to the sensor point);
    1: pinhole (the ray leaves lens_origin).  rotation: the lens-to-world 3x3 matrix; the lens looks along its local -z, the sensor lies
    at local z = sensor_distance.  blades: (n, 3, 3) aperture triangles in world space.
    Returns sensor (n, 2) sensor-plane coordinates, pixel (n, 2) real-valued pixel coordinates (px + jitter), focus (n, 3) the world point
    of the focus plane the ray passes (thin lens), blade_distance (n,): how far the origin lies outside the nearest blade (0: on one)."""
    R = np.asarray(rotation, np.float64).reshape(3, 3)
    Rinv = np.linalg.inv(R)
    o = (np.asarray(origin, np.float64) - np.asarray(lens_origin, np.float64)) @ Rinv.T
    dl = np.asarray(direction, np.float64) @ Rinv.T
    if lens_kind == 1:
        s = dl * (sensor_distance / dl[:, 2])[:, None]                       # the line through the pinhole, followed back to the sensor plane
        sensor = s[:, :2]
        focus = np.zeros_like(o)
    else:
        k = (-focus_distance - o[:, 2]) / dl[:, 2]
        F = o + k[:, None] * dl                                              # on the plane in focus, local z = -focus_distance
        sensor = (-sensor_distance / focus_distance) * F[:, :2]              # its conjugate point: the central ray through the lens centre
        focus = F @ R.T + np.asarray(lens_origin, np.float64)
    pixel = np.stack([(sensor[:, 0] / sensor_w + 0.5) * width, (sensor[:, 1] / sensor_h + 0.5) * height], 1)
    blades = np.asarray(blades, np.float64)
    dist = np.full(len(o), np.inf)
    P = np.asarray(origin, np.float64)
    for tri in blades:
        A, B, Cc = tri
        N = np.cross(B - A, Cc - A)
        if norm(N) == 0:
            dist = np.minimum(dist, norm(P - A))
            continue
        nh = N / norm(N)
        off = np.abs(dot(P - A, nh))
        inside = np.inf
        for Va, Vb in ((A, B), (B, Cc), (Cc, A)):
            e = Vb - Va
            inside = np.minimum(inside, dot(np.cross(e, P - Va), nh) / norm(e))
        dist = np.minimum(dist, np.maximum(off, np.maximum(-inside, 0.0)))
    return dict(sensor=sensor, pixel=pixel, focus=focus, blade_distance=dist)


# ------------------------------------------------------------------------------------------------------------------
# light paths: the light table, the start of a path, the lens response
# ------------------------------------------------------------------------------------------------------------------
def surface_area(kind, p):
    p = np.asarray(p, np.float64)
    if kind == TRIANGLE:
        return 0.5 * float(norm(np.cross(p[3:6] - p[:3], p[6:9] - p[:3])))
    if kind == SPHERE:
        return 4.0 * np.pi * p[3] ** 2
    if kind == DISK:
        return np.pi * p[6] ** 2
    return 2.0 * np.pi * p[6] * p[7]


def light_table(kinds, params, materials):
    """The light set of a scene, from its definition.  materials: per object the emitted radiance rho (3,), or None for an object that is no
    emitter.  Irradiance = pi rho, power = area x sum(irradiance); lights in ascending order of power (equal powers in scene order), with
    running sums.  Returns object, kind, params, irradiance (n, 3), power, cum_power, total, pdf_area = sum(irradiance) / total."""
    idx = [i for i, m in enumerate(materials) if m is not None]
    irr = np.array([np.pi * np.asarray(materials[i], np.float64) for i in idx]).reshape(len(idx), 3)
    power = np.array([surface_area(int(kinds[i]), params[i]) * irr[k].sum() for k, i in enumerate(idx)])
    order = np.argsort(power, kind="stable")
    obj = np.array(idx, np.int64)[order]
    cum = np.cumsum(power[order])
    total = float(cum[-1]) if len(cum) else 0.0
    return dict(object=obj, kind=np.asarray(kinds, np.int64)[obj], params=np.asarray(params, np.float64)[obj], irradiance=irr[order], power=power[order],
                cum_power=cum, total=total, pdf_area=irr[order].sum(1) / total if len(cum) else np.zeros(0))


LIGHT_DRAWS = 5                                    # the choice, two for the surface point, two for the direction: every kind


def light_ray(table, state, side=(0.0, False)):
    """The start of a light path for n sampler states (uint64): the light = the first one whose cumulative power >= u x total; a point of its
    surface -- triangle: barycentric (u, v), reflected to (1 - u, 1 - v) where u + v >= 1; sphere: centre + r (r0 cos phi, r0 sin phi,
    sqrt(1 - r0^2)) with r0 = 2 u - 1 in [-1, 1), which is NOT the uniform sphere (it covers z >= 0 of the local frame only); disk: centre +
    sqrt(u r^2) (a cos theta + b sin theta) on the frame (a, b) of its normal; cylinder: centre + u h axis + r (a cos theta + b sin theta) --
    then a cosine-weighted direction about the surface normal there (triangle: unit(E1 x E2); sphere, cylinder: the radial unit vector; disk:
    the normal as given); weight = irradiance / pdf_area.
    side = (b_choice, other_axis): the answer with the choice taken as if u were larger by b_choice and the direction's frame on the other
    axis.  The fold has no side: the draws are multiples of 2^-24, rounding their sum to binary32 is monotone and 1 is a binary32 number, so
    "u + v >= 1" is decided as in exact arithmetic -- also where u + v = 1 exactly.  Returns light (position in the table), object, origin,
    normal, dir, weight, draws, state (after), and the conditioning: cond_choice (|u - cum_k / total|, nearest k), cond_axis (||n.x| - |n.y||
    of the normal where it is computed), cond_root (1 - r0^2 for the sphere, where its square root is not Lipschitz), cond = their minimum."""
    b_choice, other_axis = side
    st = np.array(state, np.uint64).copy()
    n = len(st)
    b_choice = np.broadcast_to(b_choice, (n,))
    u = [xorshift_uniform(st) for _ in range(LIGHT_DRAWS)]
    cum, total = table["cum_power"], table["total"]
    edges = cum[:-1] / total                                              # the last light ends at u = 1, which is never drawn
    light = np.minimum((edges[None, :] < (u[0] + b_choice)[:, None]).sum(1), len(cum) - 1)
    cond_choice = np.abs(edges[None, :] - u[0][:, None]).min(1) if len(edges) else np.full(n, np.inf)
    origin, normal = np.zeros((n, 3)), np.zeros((n, 3))
    cond_root = np.full(n, np.inf)
    for k in range(len(cum)):
        s = light == k
        if not s.any():
            continue
        kind, p = int(table["kind"][k]), table["params"][k]
        a, b = u[1][s], u[2][s]
        if kind == TRIANGLE:
            A, B, Cc = p[:3], p[3:6], p[6:9]
            fold = a + b >= 1.0
            a, b = np.where(fold, 1.0 - a, a), np.where(fold, 1.0 - b, b)
            origin[s] = (1.0 - a - b)[:, None] * A + a[:, None] * B + b[:, None] * Cc
            normal[s] = unit(np.cross(B - A, Cc - A))
        elif kind == SPHERE:
            r0, phi = 2.0 * a - 1.0, 2.0 * np.pi * b
            root = np.sqrt(np.maximum(1.0 - r0 * r0, 0.0))
            normal[s] = np.stack([r0 * np.cos(phi), r0 * np.sin(phi), root], 1)
            origin[s] = p[:3] + p[3] * normal[s]
            cond_root[s] = 1.0 - r0 * r0
        else:
            N = np.broadcast_to(p[3:6], (int(s.sum()), 3))
            fa, fb = _frame(N)
            theta = 2.0 * np.pi * b
            ring = fa * np.cos(theta)[:, None] + fb * np.sin(theta)[:, None]
            if kind == DISK:
                origin[s] = p[:3] + ring * np.sqrt(a * p[6] * p[6])[:, None]
                normal[s] = N
            else:
                origin[s] = p[:3] + N * (a * p[7])[:, None] + ring * p[6]
                normal[s] = unit(ring)
    cond_axis = np.where(table["kind"][light] == DISK, np.inf, np.abs(np.abs(normal[:, 0]) - np.abs(normal[:, 1])))      # a disk's normal is its input: decided exactly
    d = _lobe(normal, np.sqrt(u[3]), u[4], other_axis)
    weight = table["irradiance"][light] / table["pdf_area"][light][:, None]
    return dict(light=light, object=table["object"][light], origin=origin, normal=normal, dir=d, weight=weight, draws=np.full(n, LIGHT_DRAWS), state=st,
                u=np.stack(u, 1), cond_choice=cond_choice, cond_axis=cond_axis, cond_root=cond_root,
                cond=_smin(cond_choice, cond_axis, cond_root))


def lens_response(lens_kind, lens_origin, rotation, focus_distance, sensor_distance, width, height, sensor_w, sensor_h, position, direction_out):
    """The inverse camera as the light tracer asks for it: does the ray that arrives at `position` on the lens from direction_out (pointing
    from the lens into the scene: an eye ray's own direction) reach the sensor, at which pixel, with which value?  Built on eye_ray_to_pixel.
    Thin lens: no response for a direction with local z >= 0 (from behind); value = (unit(sensor_point - aperture_point).z / direction.z)^4,
    direction as given (not normalised).  Pinhole: value 1, no refusal by sign.
    Returns reached, pixel (n, 2) real-valued, index (floor, clamped: x + y width), value, z (the local z of the direction),
    edge: the distance of the real-valued pixel position from the nearest pixel edge (sensor edges included), in pixels."""
    R = np.asarray(rotation, np.float64).reshape(3, 3)
    Rinv = np.linalg.inv(R)
    pos, do = np.asarray(position, np.float64), np.asarray(direction_out, np.float64)
    with np.errstate(all="ignore"):
        r = eye_ray_to_pixel(lens_kind, lens_origin, rotation, focus_distance, sensor_distance, np.zeros((0, 3, 3)), width, height, sensor_w, sensor_h, pos, do)
        dl = do @ Rinv.T
        pix = r["pixel"]
        size = np.array([width, height], np.float64)
        inside = np.isfinite(pix).all(1) & (pix >= 0).all(1) & (pix < size).all(1)
        if lens_kind == 1:
            reached, value = inside, np.ones(len(pos))
        else:
            reached = inside & (dl[:, 2] < 0)
            ap = (pos - np.asarray(lens_origin, np.float64)) @ Rinv.T
            sp = np.concatenate([r["sensor"], np.full((len(pos), 1), float(sensor_distance))], 1)
            value = (unit(sp - ap)[:, 2] / dl[:, 2]) ** 4
        cell = np.minimum(np.floor(np.where(np.isfinite(pix), pix, 0.0)), size - 1)
        index = np.where(reached, cell[:, 0] + cell[:, 1] * width, 0).astype(np.int64)
        edge = np.abs(pix - np.clip(np.round(pix), 0.0, size)).min(1)
        edge = np.where(np.isfinite(edge), edge, np.inf)
    return dict(reached=reached, pixel=pix, index=index, value=np.where(reached, value, 0.0), z=dl[:, 2], edge=edge)


if __name__ == "__main__":
    import sys
    if "--measure" in sys.argv:
        import f64_inputs
        f64_inputs.measure(write="--dry" not in sys.argv)
    else:
        print(__doc__)

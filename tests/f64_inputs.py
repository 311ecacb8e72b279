"""Inputs of the binary64 comparison (tests/f64_reference.py): scenes, rays aimed at decision boundaries, material items and
cameras -- shared by test_f64_reference_cpu.py, test_f64_reference_gpu.py and `python tests/f64_reference.py --measure`.
Everything is a function of fixed seeds.  Rays and scenes are binary32; an "ulp-scale step" is a step of k ulp at the scene's extent."""
import ctypes as C
import json
from functools import lru_cache
from pathlib import Path

import numpy as np

import f64_reference as R

BOUNDS_FILE = Path(__file__).parent / "golden" / "f64_reference_bounds.json"
STEPS = np.array([0, 1, -1, 4, -4, 64, -64, 4096, -4096], np.float64)
F32 = np.float32
EYE_TRANSFORM = dict(
    plain=[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 3, 0, 0, 0, 1],
    # rotation about y by 0.5 rad, then about x by 0.3 rad (orthonormal to binary32 rounding), camera off the axes
    turned=[float(F32(v)) for v in (0.87758256, 0.0, 0.47942554, 1.2, 0.14167993, 0.95533649, -0.25934339, -0.7, -0.45801188, 0.29552021, 0.83838665, 2.4, 0, 0, 0, 1)])
PRIMS = {
    R.TRIANGLE: [-0.6, -0.4, 0.1, 0.7, -0.3, -0.2, 0.1, 0.8, 0.3],
    R.SPHERE: [0.2, -0.1, 0.3, 0.45],
    R.DISK: [0.1, 0.2, -0.1, 0.3, 0.9, -0.2, 0.6],
    R.CYLINDER: [-0.2, -0.5, 0.1, 0.18814417, 0.94072087, 0.28221626, 0.35, 0.9],
}
# (name, scale, offset, direction scale, disk-normal scale, rays per half)
VARIANTS = [("base", 1.0, 0.0, 1.0, 1.0, 4000), ("dir*1e-3", 1.0, 0.0, 1e-3, 1.0, 1500), ("dir*1e3", 1.0, 0.0, 1e3, 1.0, 1500),
            ("scale 1e-2 offset 1", 1e-2, 1.0, 1.0, 1.0, 1500), ("scale 1e3 offset 1e5", 1e3, 1e5, 1.0, 1.0, 1500)]
DISK_VARIANTS = [("|normal| 0.01", 1.0, 0.0, 1.0, 0.01 / 0.9695360, 1000), ("|normal| 100", 1.0, 0.0, 1.0, 100 / 0.9695360, 1000)]
MATERIALS = [(0, (0.7, 0.6, 0.5), 0.0), (1, (0.8, 0.7, 0.6), 0.0), (1, (0.8, 0.7, 0.6), 1.0), (1, (0.8, 0.7, 0.6), 4.0), (1, (0.8, 0.7, 0.6), 256.0),
             (1, (0.8, 0.7, 0.6), 1e4), (2, (0.9, 0.8, 0.7), 0.0), (3, (1.0, 1.0, 1.0), 1.5), (3, (1.0, 1.0, 1.0), 1.33), (3, (1.0, 1.0, 1.0), 2.4),
             (4, (5.0, 4.0, 3.0), 0.0), (5, (1.0, 1.0, 1.0), 0.0)]     # the last one: the Eye material every scene appends after its own
MATERIAL_SETS = [("lambertian", R.LAMBERTIAN, [0], False), ("phong", R.PHONG, [1, 2, 3, 4, 5], False), ("specular", R.SPECULAR, [6], False),
                 ("refraction", R.REFRACTION, [7, 8, 9], False), ("refraction_importance", R.REFRACTION, [7, 8, 9], True),
                 ("diffuse_light", R.DIFFUSE_LIGHT, [10], False), ("eye", R.EYE, [11], False)]
PINHOLE = dict(transform=EYE_TRANSFORM["plain"], focal_length=0.045, focus_distance=3.0, radius=0.02, n_blades=0)
FRAMES = [(1, 1), (3, 2), (17, 8), (80, 56)]
CAMERAS = {"thin3": dict(transform=EYE_TRANSFORM["turned"], focal_length=0.05, focus_distance=2.5, radius=0.05, n_blades=3),
           "thin6": dict(transform=EYE_TRANSFORM["plain"], focal_length=0.05, focus_distance=3.0, radius=0.02, n_blades=6),
           "pinhole": dict(transform=EYE_TRANSFORM["turned"], focal_length=0.045, focus_distance=3.0, radius=0.02, n_blades=0)}
EYE_SEED, EYE_SAMPLES = 424242, 4
# A measured worst case below half an ulp is the luck of a finite sample: a correctly rounded binary32 result is already up to half an ulp
# from the binary64 value, so no quantity is held to less than 4 x 0.5 ulp.
FLOOR_ULP = 0.5


def transformed(kind, p, scale, offset, nscale=1.0):
    p = np.array(p, np.float64)
    for k in range(0, 9 if kind == R.TRIANGLE else 3, 3):
        p[k:k + 3] = p[k:k + 3] * scale + offset
    if kind == R.SPHERE:
        p[3] *= scale
    elif kind == R.DISK:
        p[3:6] *= nscale
        p[6] *= scale
    elif kind == R.CYLINDER:
        p[6:8] *= scale
    out = np.zeros(12, F32)
    out[:len(p)] = p
    return out


def _perp(rng, v):
    """random unit vectors perpendicular to the unit vectors v"""
    a = np.cross(v, rng.normal(size=v.shape))
    return R.unit(a)


def _geometry(kind, p):
    p = np.asarray(p, np.float64)
    if kind == R.TRIANGLE:
        V = p[:9].reshape(3, 3)
        return V.mean(0), max(R.norm(V[1] - V[0]), R.norm(V[2] - V[1]), R.norm(V[0] - V[2]))
    if kind == R.SPHERE:
        return p[:3], p[3]
    if kind == R.DISK:
        return p[:3], p[6]
    nh = p[3:6] / R.norm(p[3:6])
    return p[:3] + nh * p[7] / 2, max(p[6], p[7])


def random_rays(kind, p, rng, n):
    c0, L = _geometry(kind, p)
    o = c0 + rng.uniform(-3, 3, (n, 3)) * L
    d = R.unit(c0 + rng.uniform(-1.2, 1.2, (n, 3)) * L - o)
    return o, d


def aimed_rays(kind, p, rng, n):
    """Rays through points a few ulp either side of a decision boundary of the primitive (module docstring of f64_reference)."""
    p = np.asarray(p, np.float64)
    c0, L = _geometry(kind, p)
    eps = float(R.ulp32(R.extent(kind, p)))
    step = rng.choice(STEPS, n) * eps
    sel = rng.random(n)
    far = R.unit(rng.normal(size=(n, 3))) * rng.uniform(1, 3, (n, 1)) * L
    f = rng.choice([0.5, 1.0, 2.0], n) * R.KEPS                       # the kEPS family: the (far) root at t = kEPS x {0.5, 1, 2}
    if kind in (R.TRIANGLE, R.DISK):
        A = p[:3]
        if kind == R.TRIANGLE:
            V = p[:9].reshape(3, 3)
            N = np.cross(V[1] - V[0], V[2] - V[0])
            nh = N / R.norm(N)
            e = rng.integers(0, 3, n)
            Va, Vb = V[e], V[(e + 1) % 3]
            s = rng.random(n)
            s[rng.random(n) < 0.1] = 0.0                               # a vertex
            inward = R.unit(np.cross(nh, Vb - Va))
            X = Va + s[:, None] * (Vb - Va) + step[:, None] * inward
            b = rng.dirichlet([1, 1, 1], n)
            inner = b @ V
        else:
            nh = p[3:6] / R.norm(p[3:6])
            radial = _perp(rng, np.broadcast_to(nh, (n, 3)))
            X = A + (p[6] + step)[:, None] * radial
            inner = A + _perp(rng, np.broadcast_to(nh, (n, 3))) * (p[6] * np.sqrt(rng.random(n)))[:, None] * 0.9
        o = c0 + far
        o = np.where((np.abs(R.dot(o - A, nh)) < 0.05 * L)[:, None], o + 0.3 * L * nh, o)
        d = R.unit(X - o)
        ke = sel < 0.12
        dk = R.unit(rng.normal(size=(n, 3)))
        o = np.where(ke[:, None], inner - f[:, None] * dk, o)
        d = np.where(ke[:, None], dk, d)
        return o, d
    A = p[:3]
    if kind == R.SPHERE:
        r = p[3]
        nX = R.unit(rng.normal(size=(n, 3)))
        tau = _perp(rng, nX)
        o = A + (r + step)[:, None] * nX - tau * rng.uniform(0.5, 3, (n, 1)) * L      # along a tangent line of the sphere
        d = tau
        ke = sel < 0.12
        q = f / (2 * r)
        X = A + r * nX
        dk = R.unit(tau * np.sqrt(1 - q * q)[:, None] - nX * q[:, None])               # a chord of length kEPS x {0.5, 1, 2} from the surface
        return np.where(ke[:, None], X, o), np.where(ke[:, None], dk, d)
    nh = p[3:6] / R.norm(p[3:6])
    r, H = p[6], p[7]
    radial = _perp(rng, np.broadcast_to(nh, (n, 3)))
    circ = np.cross(nh, radial)
    h = rng.uniform(0, H, n)
    end = np.where(rng.random(n) < 0.5, 0.0, H)
    # (1) the two end circles, from outside
    X = A + (end + step)[:, None] * nh + r * radial
    o1 = X + (radial * rng.uniform(0.5, 2, (n, 1)) + nh * rng.uniform(-1, 1, (n, 1)) + circ * rng.uniform(-1, 1, (n, 1))) * L
    d1 = R.unit(X - o1)
    # (2) a tangent line of the lateral surface
    psi = rng.uniform(-1.2, 1.2, n)
    tau = circ * np.cos(psi)[:, None] + nh * np.sin(psi)[:, None]
    o2 = A + h[:, None] * nh + (r + step)[:, None] * radial - tau * rng.uniform(0.5, 3, (n, 1)) * L
    # (3) nearly parallel to the axis: a = eps^2 down to 1e-12, leaving the wall at an end circle or in between
    tilt = 10.0 ** -rng.integers(1, 7, n)
    z0 = rng.uniform(0.3, 1.5, n) * H
    ht = np.where(rng.random(n) < 0.6, end + step, h)
    o3 = A - z0[:, None] * nh + (r - tilt * (z0 + ht))[:, None] * radial
    d3 = R.unit(nh + tilt[:, None] * radial)
    # (4) kEPS: a chord of the cross-section from the surface
    q = f / (2 * r)
    o4 = A + h[:, None] * nh + r * radial
    d4 = R.unit(circ * np.sqrt(1 - q * q)[:, None] - radial * q[:, None])
    o = np.select([(sel < 0.4)[:, None], (sel < 0.7)[:, None], (sel < 0.88)[:, None]], [o1, o2, o3], o4)
    d = np.select([(sel < 0.4)[:, None], (sel < 0.7)[:, None], (sel < 0.88)[:, None]], [d1, tau, d3], d4)
    return o, d


@lru_cache(None)
def primitive_sets(kind):
    """[(name, scene kwargs, rays o, d (binary32), aimed mask, geometric)] of one primitive kind: one object + the pinhole's aperture triangle per scene."""
    out = []
    for vi, (name, scale, off, dscale, nscale, n) in enumerate(VARIANTS + (DISK_VARIANTS if kind == R.DISK else [])):
        rng = np.random.default_rng(1000 * kind + vi + 7)
        p = transformed(kind, PRIMS[kind], scale, off, nscale)
        ro, rd = random_rays(kind, p, rng, n)
        ao, ad = aimed_rays(kind, p, rng, n)
        o = np.concatenate([ro, ao]).astype(F32)
        d = (np.concatenate([rd, ad]) * dscale).astype(F32)
        aimed = np.arange(2 * n) >= n
        lens = dict(PINHOLE, transform=[1, 0, 0, off, 0, 1, 0, off, 0, 0, 1, off + 3 * scale, 0, 0, 0, 1])
        scene = dict(objects=[(kind, 0, [float(v) for v in p[:9]])], materials=MATERIALS[:1], **lens)
        # the reference's sphere test takes |dir| = 1 (a = 1 in its quadratic, primitive_sphere.cc:78): with a scaled direction it is not the
        # geometric test, so those two sets are compared with that property (test_sphere_takes_directions_as_unit), not with the geometry
        geometric = not (kind == R.SPHERE and dscale != 1.0)
        out.append((name, scene, o, d, aimed, geometric))
    return out


@lru_cache(None)
def mixed_set():
    """About a hundred objects of all four kinds around the origin behind a six-blade thin lens (the scene tests/lens_sanitize.hip describes,
    with unit cylinder axes): 106 objects, beyond the 80 at which AUTO leaves the two-phase engine.  10 000 random + 10 000 aimed rays."""
    state = 12345
    def u():
        nonlocal state
        state = (state * 1664525 + 1013904223) & 0xffffffff
        return float(F32((state >> 8) / 16777216.0 * 2.0 - 1.0))
    objs = []
    for i in range(100):
        kind = i % 4
        c = [2.0 * u() for _ in range(3)]
        if kind == R.TRIANGLE:
            q = [c[k] + 0.3 * u() for k in range(3)] + [c[k] + 0.3 * u() for k in range(3)]
            prm = c + q
        elif kind == R.SPHERE:
            prm = c + [0.15]
        else:
            nv = np.array([u(), u(), 1.5])
            if kind == R.CYLINDER:
                nv = nv / np.linalg.norm(nv)
            prm = c + [float(F32(v)) for v in nv] + [0.2, 0.4]
        objs.append((kind, i % 3, [float(F32(v)) for v in prm]))
    scene = dict(objects=objs, materials=[MATERIALS[0], MATERIALS[6], MATERIALS[7]], transform=[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 6, 0, 0, 0, 1],
                 focal_length=0.05, focus_distance=6.0, radius=0.05, n_blades=6)
    rng = np.random.default_rng(99)
    n = 10000
    ro = rng.uniform(-3, 3, (n, 3))
    rd = R.unit(rng.uniform(-2, 2, (n, 3)) - ro)
    ao, ad = [], []
    for kind, _, prm in objs:
        a, b = aimed_rays(kind, np.array(prm + [0.0] * (12 - len(prm))), rng, n // 100)
        ao.append(a); ad.append(b)
    o = np.concatenate([ro] + ao).astype(F32)
    d = np.concatenate([rd] + ad).astype(F32)
    return scene, o, d, np.arange(2 * n) >= n


def scene_arrays(osc):
    """(kinds, params (n, 12) float64) of an oracle scene, the aperture blades included."""
    objs = osc.objects()
    kinds = np.array([k for k, *_ in objs], np.int64)
    params = np.zeros((len(objs), 12))
    for i, (_, _, p, _) in enumerate(objs):
        params[i, :9] = p
    return kinds, params


@lru_cache(None)
def material_items(name):
    """4 000 items of one material set: (kind, material indices, importance, material index per item, normals, dir_out, states)."""
    _, kind, mats, importance = next(s for s in MATERIAL_SETS if s[0] == name)
    rng = np.random.default_rng(21 + sum(map(ord, name)))
    n = 4000
    mat = np.array(mats)[np.arange(n) % len(mats)].astype(np.uint32)
    nrm = R.unit(rng.normal(size=(n, 3)))
    do = R.unit(rng.normal(size=(n, 3)))
    do[:1000] = R.unit(nrm[:1000] * 0.05 + do[:1000])
    tang = _perp(rng, nrm)
    g = slice(1000, 1300)                                              # grazing: |cos| <= 1e-4
    do[g] = R.unit(tang[g] + nrm[g] * rng.uniform(-1e-4, 1e-4, (300, 1)))
    e = slice(1300, 1400)                                              # exactly tangent: axis normals, dir_out in the plane (the product is exactly 0)
    axis = rng.integers(0, 3, 100)
    nrm[e] = np.eye(3)[axis] * rng.choice([-1.0, 1.0], (100, 1))
    phi = rng.uniform(0, 2 * np.pi, 100)
    do[e] = np.eye(3)[(axis + 1) % 3] * np.cos(phi)[:, None] + np.eye(3)[(axis + 2) % 3] * np.sin(phi)[:, None]
    if kind == R.REFRACTION:                                           # the critical angle of each ior, +- a few ulp, from inside
        c = slice(1400, 2000)
        ior = np.array([MATERIALS[m][2] for m in mat[c]])
        step = np.where(np.arange(600) % 2 == 0, rng.choice([0, 1, -1, 2, -2, 8, -8, 64, -64], 600) * 2.0 ** -24,      # a few ulp of the angle ...
                        rng.choice([-1.0, 1.0], 600) * 10.0 ** rng.uniform(-3.5, -1.5, 600))                          # ... and clearly on either side
        alpha = np.arcsin(1.0 / ior) + step
        do[c] = tang[c] * np.sin(alpha)[:, None] - nrm[c] * np.cos(alpha)[:, None]
    state = rng.integers(1, 2 ** 63, n).astype(np.uint64)
    return kind, mats, importance, mat, nrm.astype(F32), do.astype(F32), state


def material_reference(name, side=(0, 0, 0, False), margins=None, follow=None):
    """The binary64 answer for every item of a set.  side = (-1 | 0 | 1, -1 | 0 | 1, -1 | 0 | 1, other axis): the answer on one side of the
    decisions (f64_reference.sample_material), each biased by that sign x margins[material index]."""
    kind, mats, importance, mat, nrm, do, state = material_items(name)
    ref = None
    for m in mats:
        sel = mat == m
        rho, prm = MATERIALS[m][1], float(F32(MATERIALS[m][2]))
        part = R.sample_material(kind, np.array(rho, F32).astype(np.float64), prm, nrm[sel].astype(np.float64), do[sel].astype(np.float64), state[sel], importance,
                                 (0.0, 0.0, 0.0, False) if margins is None else (side[0] * margins[m], side[1] * margins[m], side[2] * margins[m], side[3]),
                                 None if follow is None else follow[sel])
        if ref is None:
            ref = {k: np.zeros((len(mat),) + v.shape[1:], v.dtype) for k, v in part.items()}
        for k, v in part.items():
            ref[k][sel] = v
    return ref


# ------------------------------------------------------------------------------------------------------------------
# the oracle on these inputs (CPU)
# ------------------------------------------------------------------------------------------------------------------
def oracle_casts(osc, o, d):
    """Scene.cast of every ray: (object or -1, t, pos, normal)."""
    n = len(o)
    obj, t, pos, nrm = np.empty(n, np.int32), np.empty(n, F32), np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    for i in range(n):
        obj[i], t[i], pos[i], nrm[i] = osc.cast(o[i], d[i])
    return obj, t, pos, nrm


def oracle_materials(name):
    import oracle_binding as O
    L = O.load()
    kind, mats, importance, mat, nrm, do, state = material_items(name)
    n = len(mat)
    di, w, used = np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.zeros(n, np.int64)
    oms = {m: O.OMaterial(MATERIALS[m][0], (C.c_float * 3)(*MATERIALS[m][1]), MATERIALS[m][2]) for m in mats}
    for i in range(n):
        used[i] = L.oracle_sample_material_xorshift(C.byref(oms[int(mat[i])]), nrm.ctypes.data + 12 * i, do.ctypes.data + 12 * i, int(state[i]),
                                                    int(importance), O.MATH_GLIBC, di.ctypes.data + 12 * i, w.ctypes.data + 12 * i)
    return di, w, used


def camera_scene(name):
    return dict(objects=[(R.SPHERE, 0, [0.0, 0.0, 0.0, 0.3])], materials=MATERIALS[:1], **CAMERAS[name])


def eye_items(W, H):
    px = np.repeat(np.arange(W * H, dtype=np.uint32), EYE_SAMPLES)
    sm = np.tile(np.arange(EYE_SAMPLES, dtype=np.uint32), W * H)
    return px, sm


def oracle_eye(osc, W, H):
    px, sm = eye_items(W, H)
    out = np.zeros((len(px), 7), F32)
    for i in range(len(px)):
        _, _, e = osc.trace(W, H, EYE_SEED, int(px[i] % W), int(px[i] // W), int(sm[i]), max_bounces=1)
        out[i] = e
    return out


def eye_reference(osc, name, W, H, eye):
    """Errors of the eye rays `eye` (n, 7) of frame W x H: how far outside its pixel's rectangle each ray lands (in ulp of the frame's larger
    side, pixel units), how far its origin is from the nearest blade (ulp of the lens position / aperture), how far it passes from the
    nearest point of the pixel's conjugate rectangle on the focus plane (ulp of the focus distance)."""
    import oracle_binding as O
    cam = CAMERAS[name]
    kind = 1 if cam["n_blades"] == 0 else 0
    T = np.array([float(F32(v)) for v in cam["transform"]]).reshape(4, 4)
    origin, g = T[:3, 3].astype(F32), T[:3, :3]
    f, fd = float(F32(cam["focal_length"])), float(F32(cam["focus_distance"]))
    sd = f if kind == 1 else 1.0 / (1.0 / f - 1.0 / fd)                   # the thin-lens equation; the pinhole's focal length IS its sensor distance
    objs = osc.objects()
    blades = np.array([p[:9].reshape(3, 3) for _, _, p, _ in objs[:max(1, cam["n_blades"])]], np.float64)
    s = O.sensor(W, H)
    px, sm = eye_items(W, H)
    r = R.eye_ray_to_pixel(kind, origin.astype(np.float64), g.astype(np.float64), float(fd), float(sd), blades, W, H,
                           float(s.scene_width), float(s.scene_height), eye[:, :3], eye[:, 3:6])
    pix = np.stack([px % W, px // W], 1).astype(np.float64)
    over = np.maximum(np.maximum(pix - r["pixel"], r["pixel"] - (pix + 1)), 0.0)
    out = dict(pixel=over.max(1) / R.ulp32(max(W, H)), found=np.floor(r["pixel"]), want=pix,
               blade=r["blade_distance"] / R.ulp32(max(np.abs(origin).max(), cam["radius"])))
    if kind == 0:
        scale = np.array([float(s.scene_width) / W, float(s.scene_height) / H]) * float(fd) / float(sd)      # a pixel's side on the focus plane
        out["focus"] = (over * scale).max(1) / R.ulp32(float(fd))
    else:
        out["focus"] = np.zeros(len(px))
        out["pinhole_origin"] = np.abs(eye[:, :3] - origin).max(1)
    return out


# ------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------
def load_bounds():
    """The bounds in force: 4 x the measured worst case of every quantity (tests/golden/f64_reference_bounds.json)."""
    m = json.loads(BOUNDS_FILE.read_text())["measured_ulp"]
    scale = lambda d: {k: (scale(v) if isinstance(v, dict) else R.BOUND_FACTOR * max(v, FLOOR_ULP)) for k, v in d.items()}
    return scale(m)


def intersect_errors(osc, o, d, bounds):
    kinds, params = scene_arrays(osc)
    c = R.with_radius(R.scene_candidates(kinds, params, o, d), kinds, params)
    obj, t, pos, nrm = oracle_casts(osc, o, d)
    return c, (obj, t, pos, nrm), R.judge(c, obj, t, pos, nrm, bounds, o, d)


def residual_ulp(kinds, params, obj, pos):
    """How far pos lies from the surface of object obj (its implicit equation), in ulp of max(|pos|, the object's extent); 0 for a miss."""
    out = np.zeros(len(obj))
    for oi in np.unique(obj[obj >= 0]):
        r = obj == oi
        k = int(kinds[oi])
        out[r] = R.residual(k, params[oi], pos[r].astype(np.float64)) / R.ulp32(np.maximum(np.abs(pos[r]).max(1), R.extent(k, params[oi])))
    return out


def material_errors(ref, di, w):
    e_dir = np.abs(di.astype(np.float64) - ref["dir_in"]).max(1) / 2.0 ** -23
    e_w = (np.abs(w.astype(np.float64) - ref["weight"]) / R.ulp32(np.maximum(np.abs(ref["weight"]), 1.0))).max(1)
    return e_dir, e_w


def material_bounds(bounds, name, mat):
    """Per item: the bounds of dir_in and weight (ulp of 1) of its material, and the conditioning margin they imply (4 x the larger, absolute)."""
    b_dir = np.array([bounds[name][str(m)]["dir_in"] for m in mat])
    b_w = np.array([bounds[name][str(m)]["weight"] for m in mat])
    return b_dir, b_w, R.MARGIN_FACTOR * np.maximum(b_dir, b_w) * 2.0 ** -23


def material_classify(name, di, w, used, bounds):
    """For every item: does (dir_in, weight, draws) equal, within the bounds, the binary64 answer on SOME side of the decisions that lie within
    the margin?  A transmitted direction within the margin of total reflection gets the width of the interval cos(beta) can lie in when
    sin^2(beta) is known to the margin (the square root is not Lipschitz at 0) on top of its bound."""
    kind, mats, importance, mat, nrm, do, state = material_items(name)
    b_dir, b_w, margin = material_bounds(bounds, name, mat)
    margins = {m: float(margin[mat == m][0]) for m in mats}
    ok = np.zeros(len(mat), bool)
    sides = [(0, 0, 0, False)] + [(a, b, c, f) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1) for f in (False, True)]
    runs = [(side, None) for side in sides]
    if kind == R.PHONG:                                                   # any pattern of rejections the margin allows, ending where the implementation ended
        runs += [((0, 0, 1, f), used // 2) for f in (False, True)]
    for side, follow in runs:
        ref = material_reference(name, side, margins, follow)
        e_dir, e_w = material_errors(ref, di, w)
        extra = 0.0
        if kind == R.REFRACTION:
            c2 = 1.0 - ref["sin2_beta"]
            extra = np.where(ref["reflect"], 0.0, np.sqrt(np.maximum(c2, 0.0) + margin) - np.sqrt(np.maximum(c2 - margin, 0.0))) / 2.0 ** -23
            extra = np.where(np.abs(c2) <= margin, extra, 0.0)
        with np.errstate(invalid="ignore"):
            ok |= (used == ref["draws"]) & (e_dir <= b_dir + extra) & (e_w <= b_w) & (True if follow is None else ref["follow_valid"])
    return ok


def material_well(ref, margin):
    """Items farther than the margin from every discontinuity of the answer."""
    return ref["cond"] > margin


def measure(write=True):
    """Oracle against binary64 on every input above: the worst error per quantity over the inputs the CURRENT bounds call well-conditioned,
    iterated until the bounds (4 x worst) and the margins (4 x bounds) they imply reproduce themselves."""
    import oracle_binding as O
    measured = {"intersect": {}, "material": {}, "eye": {}}
    start = {k: {"t": 16.0, "pos": 16.0, "normal": 16.0, "residual": 16.0} for k in R.KIND_NAMES}
    shares = {}
    scenes = [(R.KIND_NAMES[kind] + " / " + name, kind, O.Scene.create(**scene), o, d, aimed) for kind in range(4) for name, scene, o, d, aimed, geo in primitive_sets(kind) if geo]
    msc, mo, md, maimed = mixed_set()
    scenes.append(("mixed", -1, O.Scene.create(**msc), mo, md, maimed))
    for name, kind, osc, o, d, aimed in scenes:
        kinds, params = scene_arrays(osc)
        cur = start
        for it in range(6):
            b = {k: {q: R.BOUND_FACTOR * max(v, FLOOR_ULP) for q, v in qs.items()} for k, qs in cur.items()}
            worst = {k: {"t": 0.0, "pos": 0.0, "normal": 0.0, "residual": 0.0} for k in R.KIND_NAMES if (kinds == R.KIND_NAMES.index(k)).any()}
            c, (obj, t, pos, nrm), j = intersect_errors(osc, o, d, {**start, **b})
            shares[name] = float((~j["well"][~aimed]).mean())
            hit = (obj >= 0) & j["well"]
            for k in range(4):
                s = hit & (kinds[np.maximum(obj, 0)] == k)
                if not s.any():
                    continue
                w = worst[R.KIND_NAMES[k]]
                for q, e in (("t", j["err_t"]), ("pos", j["err_pos"]), ("normal", j["err_normal"])):
                    w[q] = max(w[q], float(e[s].max()))
                w["residual"] = max(w["residual"], float(residual_ulp(kinds, params, obj, pos)[s].max()))
            if worst == cur:
                break
            cur = worst
        measured["intersect"][name] = cur
    for name, kind, mats, _ in MATERIAL_SETS:
        ref = material_reference(name)
        di, w, used = oracle_materials(name)
        mat = material_items(name)[3]
        e_dir, e_w = material_errors(ref, di, w)
        measured["material"][name] = {}
        ill = 0
        for m in mats:                                                    # per material: a Phong exponent or an ior has its own worst case
            sel = mat == m
            cur = {"dir_in": 2.0, "weight": 2.0}
            for _ in range(6):
                margin = R.MARGIN_FACTOR * R.BOUND_FACTOR * max(cur["dir_in"], cur["weight"], FLOOR_ULP) * 2.0 ** -23
                well = sel & material_well(ref, margin) & (used == ref["draws"])
                new = {"dir_in": float(e_dir[well].max()), "weight": float(e_w[well].max())}
                if new == cur:
                    break
                cur = new
            measured["material"][name][str(m)] = cur
            ill += int((sel & ~well).sum())
        shares["material / " + name] = ill / len(mat)
    for cam in CAMERAS:
        osc = O.Scene.create(**camera_scene(cam))
        worst = {"pixel": 0.0, "blade": 0.0, "focus": 0.0}
        for W, H in FRAMES:
            e = eye_reference(osc, cam, W, H, oracle_eye(osc, W, H))
            for q in worst:
                worst[q] = max(worst[q], float(e[q].max()))
        measured["eye"][cam] = worst
    doc = {"_": "Largest error of the oracle against tests/f64_reference.py on the inputs of tests/f64_inputs.py, in ulp (python tests/f64_reference.py --measure). "
                "Data only: the tests use 4 x these as bounds and 4 x the bounds as ill-conditioning margins.",
           "measured_ulp": measured, "ill_conditioned_share_of_random_half": shares}
    print(json.dumps(doc, indent=1))
    if write:
        BOUNDS_FILE.write_text(json.dumps(doc, indent=1) + "\n")
    return doc

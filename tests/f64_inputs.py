"""Inputs of the binary64 comparison (tests/f64_reference.py): scenes, rays aimed at decision boundaries, material items,
cameras, light sets (sampler states aimed at the decisions of a light path's start) and lens-response rays -- shared by test_f64_reference_cpu.py, test_f64_reference_gpu.py and `python tests/f64_reference.py --measure`.
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
# light paths: sampler states aimed at the decisions of the light's start, rays aimed at the decisions of the lens response
# ------------------------------------------------------------------------------------------------------------------
U64 = np.uint64
LIGHT_STEPS = np.array([0, 1, -1, 4, -4], np.int64)                       # steps of one draw: 2^-24
LIGHT_N = 1000                                                            # items per half of a light set
F_RANDOM, F_CHOICE, F_FOLD, F_R0, F_HEMI, F_PHI, F_INSIDE = 0, 1, 2, 3, 4, 5, 6          # F_INSIDE: the middle of every light's interval (no boundary)
LIGHT_FAMILIES = {F_CHOICE: "choice", F_FOLD: "fold", F_R0: "sphere r0", F_HEMI: "hemisphere r0", F_PHI: "phi"}
LIGHT_MATERIALS = [(0, (0.7, 0.6, 0.5), 0.0), (4, (5.0, 4.0, 3.0), 0.0), (4, (0.25, 0.0, 2.0), 0.0), (4, (300.0, 200.0, 100.0), 0.0), (4, (0.001, 0.002, 0.003), 0.0)]
LIGHT_VARIANTS = [("base", 1.0, 0.0), ("scale 1e-2 offset 1", 1e-2, 1.0), ("scale 1e3", 1e3, 0.0), ("scale 1e3 offset 1e5", 1e3, 1e5)]
LIGHT_SET_NAMES = [k + " / " + v[0] for k in R.KIND_NAMES for v in LIGHT_VARIANTS] + [f"mixed / {n}" for n in (1, 2, 5, 40)]
SMALL_N = (1, 63, 64, 65, 257)                                            # the launch's wave and block boundaries (GPU leg, base triangle set)


def xorshift_back(state):
    """The state one step before: the inverse of f64_reference.xorshift_uniform's step (each of its three shifts-and-xors is undone by a
    product of shifts-and-xors by the doubled distances)."""
    s = np.array(state, U64).copy()
    for k in (17, 34):
        s ^= s << U64(k)
    for k in (7, 14, 28, 56):
        s ^= s >> U64(k)
    for k in (13, 26, 52):
        s ^= s << U64(k)
    return s


def states_with_draw(rng, k, value):
    """States whose k-th draw (k = 0: the first) is value x 2^-24 (value: integers in [0, 2^24)); every other draw is whatever follows."""
    s = (np.asarray(value, np.int64).astype(U64) << U64(40)) | rng.integers(0, 1 << 40, len(value)).astype(U64)
    s[s == 0] = U64(1)
    for _ in range(k + 1):
        s = xorshift_back(s)
    return s


@lru_cache(None)
def _pair_basis():
    """The step of the sampler is linear over GF(2): for the 40 low bits of a state, what they contribute to the top 24 bits of the next
    one, reduced to an echelon basis [(pivot bit, 24-bit vector, 40-bit combination)], highest pivot first."""
    basis = {}
    for j in range(40):
        st = np.array([1 << j], U64)
        R.xorshift_uniform(st)
        v, c = int(st[0]) >> 40, 1 << j
        while v:
            top = v.bit_length() - 1
            if top not in basis:
                basis[top] = (v, c)
                break
            v, c = v ^ basis[top][0], c ^ basis[top][1]
    assert len(basis) == 24                                               # full rank: every pair of consecutive draws exists
    return [(b,) + basis[b] for b in sorted(basis, reverse=True)]


def states_with_draw_pair(k, first, second):
    """States whose k-th and (k + 1)-th draws are first x 2^-24 and second x 2^-24."""
    a, b = np.asarray(first, np.int64).astype(U64), np.asarray(second, np.int64).astype(U64)
    hi = a << U64(40)
    nxt = hi.copy()
    R.xorshift_uniform(nxt)
    t = (nxt >> U64(40)) ^ b                                              # what the low bits have to contribute
    low = np.zeros(len(a), U64)
    for bit, v, c in _pair_basis():
        m = ((t >> U64(bit)) & U64(1)).astype(bool)
        t = np.where(m, t ^ U64(v), t)
        low = np.where(m, low ^ U64(c), low)
    assert not t.any()
    s = hi | low
    for _ in range(k + 1):
        s = xorshift_back(s)
    return s


def _plane(nrm):
    a = np.cross(nrm, [0.0, 0.0, 1.0] if abs(nrm[2]) < 0.9 else [1.0, 0.0, 0.0])
    a /= np.linalg.norm(a)
    return a, np.cross(nrm, a)


def light_normals():
    """Unit normals (to binary32 rounding): one generic, one with |n.x| = |n.y| exactly, four within a few ulp of it -- the frame-axis decision."""
    h, c = F32(0.5), F32(np.sqrt(0.5))
    up = lambda x, k: np.nextafter(x, F32(2 * k), dtype=F32) if abs(k) == 1 else F32(x + k * np.spacing(x))
    return [np.array(v, F32) for v in ([0.18814417, 0.94072087, 0.28221626], [h, h, c], [h, up(h, 1), -c], [-h, up(h, -1), c], [up(h, 3), -h, c], [up(h, -3), h, -c])]


def kind_light_objects(kind, scale, off):
    """Six lights of one kind (three spheres) with the normals of light_normals(), around the origin x scale + off."""
    objs = []
    for i, nrm in enumerate(light_normals()):
        c = np.array([0.9 * (i % 3) - 0.9, 0.8 * (i // 3) - 0.4, 0.3 * i - 0.7])
        size = 0.6 if i == 0 else 0.3 * (1.0 + 0.15 * i)                # light 0 carries the power: the random half meets the others' normals rarely,
        mat = 3 if i == 0 else 2 + 2 * (i % 2)                            # the aimed half (F_CHOICE, F_INSIDE) all the time
        n64 = nrm.astype(np.float64)
        if kind == R.TRIANGLE:
            a, b = _plane(n64 / np.linalg.norm(n64))
            if i == 1:                                                    # E1 x E2 = (-1, -1, 0) size^2 exactly: |n.x| = |n.y| where the vertices are exact
                c, a, b, size = np.array([0.25, 0.5, -0.25]), np.array([1.0, -1.0, 0.0]), np.array([0.0, 0.0, 1.0]), 0.5
            p = np.concatenate([c, c + size * a, c + size * b])
        elif kind == R.SPHERE:
            if i >= 3:
                continue
            p = np.concatenate([c, [size]])
        else:
            p = np.concatenate([c, n64, [size, 1.7 * size]])
        objs.append((kind, mat, [float(v) for v in transformed(kind, p, scale, off)[:9]]))
    return objs


def mixed_light_objects(n):
    """n lights of all four kinds: powers over six decades (sizes over two, materials over five), all distinct for n = 40; for n <= 5 the
    first two are spheres of one radius and one material: exactly equal powers, in either arithmetic."""
    rng = np.random.default_rng(4100 + n)
    normals = light_normals()
    objs = []
    for i in range(n):
        kind = [R.SPHERE, R.SPHERE, R.TRIANGLE, R.DISK, R.CYLINDER][i] if i < 5 else i % 4
        c = rng.uniform(-2, 2, 3)
        size = 0.25 if i < 2 and n <= 5 else float(10.0 ** rng.uniform(-1.5, 0.5))
        mat = 1 if i < 2 else 1 + int(rng.integers(0, 4))
        nrm = normals[i % len(normals)].astype(np.float64)
        if kind == R.TRIANGLE:                                            # (a computed normal near |n.x| = |n.y| is ill-conditioned as a whole: the kind scenes have those)
            a, b = _plane(R.unit(rng.normal(size=(1, 3)))[0])
            p = np.concatenate([c, c + size * a, c + 0.8 * size * b])
        elif kind == R.SPHERE:
            p = np.concatenate([c, [size]])
        else:
            p = np.concatenate([c, nrm, [size, 1.3 * size]])
        objs.append((kind, mat, [float(v) for v in transformed(kind, p, 1.0, 0.0)[:9]]))
    objs.insert(1, (R.SPHERE, 0, [3.0, 3.0, 3.0, 0.2]))                   # an object that emits nothing, between the lights
    return objs


def light_scene_table(scene):
    """The binary64 light table of a scene description (through the oracle's object list: aperture blades and the Eye material included)."""
    import oracle_binding as O
    osc = O.Scene.create(**scene)
    kinds, params = scene_arrays(osc)
    mats = osc.materials()
    rho = [mats[m][1].astype(np.float64) if mats[m][0] == R.DIFFUSE_LIGHT else None for _, m, _, _ in osc.objects()]
    return R.light_table(kinds, params, rho), kinds, params


def _aimed_light_states(rng, table, n):
    """States aimed at the decisions of light_ray, and the family of each."""
    n_cum = len(table["cum_power"])
    kinds = set(int(k) for k in table["kind"])
    fams = [F_HEMI, F_PHI] + ([F_CHOICE, F_CHOICE, F_INSIDE] if n_cum > 1 else []) + ([F_FOLD] if R.TRIANGLE in kinds else []) + ([F_R0] if R.SPHERE in kinds else [])
    fam = np.array(fams)[np.arange(n) % len(fams)]
    st = np.zeros(n, U64)
    one = 1 << 24
    for f in set(fams):
        s = np.nonzero(fam == f)[0]
        m = len(s)
        step = LIGHT_STEPS[np.arange(m) % len(LIGHT_STEPS)]
        if f == F_CHOICE:                                                 # the first draw around every cumulative boundary (and on the nearest draw to it)
            edge = (table["cum_power"][:-1] / table["total"])[(np.arange(m) // len(LIGHT_STEPS)) % (n_cum - 1)]
            st[s] = states_with_draw(rng, 0, np.clip(np.round(edge * one).astype(np.int64) + step, 0, one - 1))
        elif f == F_INSIDE:
            mid = ((np.concatenate([[0.0], table["cum_power"][:-1]]) + table["cum_power"]) / (2 * table["total"]))[np.arange(m) % n_cum]
            st[s] = states_with_draw(rng, 0, np.clip(np.round(mid * one).astype(np.int64), 0, one - 1))
        elif f == F_FOLD:                                                 # u + v = 1 exactly and one step either side
            a = rng.integers(1, one - 1, m)
            st[s] = states_with_draw_pair(1, a, one - a + np.array([0, 1, -1])[np.arange(m) % 3])
        elif f == F_R0:                                                   # r0 = 2 u - 1 at its ends: -1, -1 + 2^-23 ... and 1 - 2^-23 ...
            near = np.arange(m) % 8
            st[s] = states_with_draw(rng, 1, np.where(np.arange(m) % 2 == 0, near // 2, one - 1 - near // 2))
        elif f == F_HEMI:                                                 # HemispherePSA's r0 nearest 0 and nearest 1
            near = np.array([0, 1, 2, 4])[(np.arange(m) // 2) % 4]
            st[s] = states_with_draw(rng, 3, np.where(np.arange(m) % 2 == 0, near, one - 1 - near))
        else:                                                             # phi at the octant boundaries of the sine and cosine: the direction's, and the surface point's
            octant = (np.arange(m) // len(LIGHT_STEPS)) % 8
            value = (octant * (one // 8) + step) % one
            which = np.where((np.arange(m) // 40) % 2 == 0, 4, 2)
            for k in (2, 4):
                st[s[which == k]] = states_with_draw(rng, k, value[which == k])
    return st, fam


@lru_cache(None)
def light_sets():
    """[(name, scene, states (uint64), aimed mask, family)]: one scene per light kind and variant, and the mixed tables of 1, 2, 5 and 40 lights.
    Each set is LIGHT_N random states and LIGHT_N aimed ones."""
    out = []
    scenes = [(R.KIND_NAMES[kind] + " / " + name, dict(objects=kind_light_objects(kind, scale, off), materials=LIGHT_MATERIALS,
                                                      **dict(PINHOLE, transform=[1, 0, 0, off, 0, 1, 0, off, 0, 0, 1, off + 30 * scale, 0, 0, 0, 1])))
              for kind in range(4) for name, scale, off in LIGHT_VARIANTS]
    scenes += [(f"mixed / {n}", dict(objects=mixed_light_objects(n), materials=LIGHT_MATERIALS, **dict(PINHOLE, transform=[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 30, 0, 0, 0, 1])))
               for n in (1, 2, 5, 40)]
    assert [name for name, _ in scenes] == LIGHT_SET_NAMES
    for si, (name, scene) in enumerate(scenes):
        rng = np.random.default_rng(7100 + si)
        table = light_scene_table(scene)[0]
        random = rng.integers(1, 2 ** 63, LIGHT_N).astype(U64)
        aimed, fam = _aimed_light_states(rng, table, LIGHT_N)
        out.append((name, scene, np.concatenate([random, aimed]), np.arange(2 * LIGHT_N) >= LIGHT_N, np.concatenate([np.zeros(LIGHT_N, np.int64), fam])))
    return out


def light_side(fam, ref, table):
    """For the aimed items: on which side of its family's boundary the binary64 answer lies (True / False)."""
    u = ref["u"]
    edges = np.concatenate([table["cum_power"][:-1] / table["total"], [np.inf]])
    nearest = edges[np.argmin(np.abs(edges[None, :] - u[:, :1]), 1)]
    off = lambda x: (x * 8.0 + 0.5) % 1.0 - 0.5                            # signed distance from the nearest octant boundary, in octants
    phi = np.where(np.abs(off(u[:, 2])) < np.abs(off(u[:, 4])), off(u[:, 2]), off(u[:, 4]))
    return np.select([fam == F_CHOICE, fam == F_FOLD, fam == F_R0, fam == F_HEMI], [u[:, 0] > nearest, u[:, 1] + u[:, 2] >= 1.0, u[:, 1] >= 0.5, u[:, 3] >= 0.5], phi >= 0.0)


def light_scale(table, ref, origin):
    """The magnitude whose ulp the origin's error is taken in: the chosen light's extent, or the origin's own."""
    ext = np.array([R.extent(int(k), p) for k, p in zip(table["kind"], table["params"])])
    return np.maximum(ext[ref["light"]], np.abs(np.asarray(origin, np.float64)).max(1))


def light_errors(table, ref, origin, direction, weight):
    """Errors against the binary64 answer `ref`, in ulp: origin (of light_scale), dir (of 1), weight (of itself), and the origin's distance
    from the surface of the chosen light (of light_scale)."""
    o64 = np.asarray(origin, np.float64)
    u = R.ulp32(light_scale(table, ref, origin))
    with np.errstate(all="ignore"):
        e_o = np.abs(o64 - ref["origin"]).max(1) / u
        e_d = np.abs(np.asarray(direction, np.float64) - ref["dir"]).max(1) / 2.0 ** -23
        e_w = (np.abs(np.asarray(weight, np.float64) - ref["weight"]) / R.ulp32(ref["weight"])).max(1)
        res = np.zeros(len(o64))
        for k in np.unique(ref["light"]):
            s = ref["light"] == k
            res[s] = R.residual(int(table["kind"][k]), table["params"][k], o64[s]) / u[s]
    nan = lambda e: np.where(np.isnan(e), np.inf, e)
    return dict(origin=nan(e_o), dir=nan(e_d), weight=nan(e_w), residual=nan(res))


LIGHT_QUANTITIES = ("residual", "origin", "dir", "weight")


def light_item_bounds(bounds, table, ref):
    """Per item, by the kind of its light: the bound of every quantity (ulp)."""
    names = [R.KIND_NAMES[k] for k in table["kind"][ref["light"]]]
    return {q: np.array([bounds[nm][q] for nm in names]) for q in LIGHT_QUANTITIES}


def light_margin(bounds, table):
    """The conditioning margin of a light table: 4 x the largest bound of origin and dir (ulp of 1, absolute) over the kinds it holds."""
    return R.MARGIN_FACTOR * max(max(bounds[R.KIND_NAMES[k]]["origin"], bounds[R.KIND_NAMES[k]]["dir"]) for k in set(int(k) for k in table["kind"])) * 2.0 ** -23


def light_classify(table, states, got, bounds):
    """For every item: is (object, origin, dir, weight, draws) within the bounds of the binary64 answer on SOME side of the decisions within
    the margin (the neighbouring light, the other frame axis; the fold is decided exactly)?  Near the sphere's rim the square root of 1 - r0^2 gets the
    width of the interval it can lie in when its argument is known to the margin."""
    origin, direction, weight, obj, used = got
    margin = light_margin(bounds, table)
    ok = np.zeros(len(states), bool)
    for sc in (0, -1, 1):
        for axis in (False, True):
            ref = R.light_ray(table, states, (sc * margin, axis))
            e = light_errors(table, ref, origin, direction, weight)
            b = light_item_bounds(bounds, table, ref)
            x = ref["cond_root"]
            with np.errstate(invalid="ignore"):
                extra = np.where(x <= margin, (np.sqrt(np.maximum(x, 0) + margin) - np.sqrt(np.maximum(x - margin, 0))) / 2.0 ** -23, 0.0)
            ok |= ((ref["cond_axis"] <= margin) | (not axis)) & (obj == ref["object"]) & (used == ref["draws"]) & (e["origin"] <= b["origin"] + extra) \
                & (e["dir"] <= b["dir"] + extra) & (e["weight"] <= b["weight"]) & (e["residual"] <= b["residual"] + extra)
    return ok


def oracle_light(osc, states):
    """(origin, dir, weight, object, draws used) of the oracle for every state."""
    import oracle_binding as O
    o, d, w, obj, after = osc.light_rays(states, math=O.MATH_GLIBC)
    return o, d, w, obj.astype(np.int64), draws_between(states, after)


def draws_between(before, after, most=16):
    """How many steps of the sampler lie between the two states (-1: more than `most`)."""
    s = np.array(before, U64).copy()
    used = np.full(len(s), -1, np.int64)
    for k in range(most + 1):
        used[(used < 0) & (s == after)] = k
        R.xorshift_uniform(s)
    return used


# ---- lens response ---------------------------------------------------------------------------------------------
RESPONSE_N = 1000
G_RANDOM, G_EDGE_X, G_EDGE_Y, G_SENSOR, G_CORNER, G_Z = 0, 1, 2, 3, 4, 5
RESPONSE_FAMILIES = {G_EDGE_X: "pixel edge in x", G_EDGE_Y: "pixel edge in y", G_SENSOR: "sensor edge", G_CORNER: "corner", G_Z: "local z = 0"}


def camera_geometry(osc, cam):
    """(kind, origin, rotation, focus distance, sensor distance, blades) of a camera in binary64, from its description (as eye_reference)."""
    c = CAMERAS[cam]
    kind = 1 if c["n_blades"] == 0 else 0
    T = np.array([float(F32(v)) for v in c["transform"]]).reshape(4, 4)
    f, fd = float(F32(c["focal_length"])), float(F32(c["focus_distance"]))
    sd = f if kind == 1 else 1.0 / (1.0 / f - 1.0 / fd)
    blades = np.array([p[:9].reshape(3, 3) for _, _, p, _ in osc.objects()[:max(1, c["n_blades"])]], np.float64)
    return kind, T[:3, 3].copy(), T[:3, :3].copy(), fd, sd, blades


def response_reference(osc, cam, W, H, pos, do):
    import oracle_binding as O
    kind, origin, g, fd, sd, _ = camera_geometry(osc, cam)
    s = O.sensor(W, H)
    return R.lens_response(kind, origin, g, fd, sd, W, H, float(s.scene_width), float(s.scene_height), pos, do)


@lru_cache(None)
def response_items(cam, W, H):
    """(position, direction_out (binary32), aimed mask, family, boundary (axis, value) per aimed item, outside-the-contract mask) of one camera
    and frame: RESPONSE_N random rays (on the blades, directions over the whole sphere) and RESPONSE_N aimed ones, built in binary64 so that
    they image STEPS ulp (of the frame's larger side, in pixels) either side of a pixel edge, a sensor edge or a corner, or have a local z of
    STEPS ulp of 1 around 0."""
    import oracle_binding as O
    osc = O.Scene.create(**camera_scene(cam))
    kind, origin, g, fd, sd, blades = camera_geometry(osc, cam)
    sn = O.sensor(W, H)
    sw, sh = float(sn.scene_width), float(sn.scene_height)
    rng = np.random.default_rng(9000 + 97 * list(CAMERAS).index(cam) + W)
    n = 2 * RESPONSE_N
    if kind == 1:
        pos = np.broadcast_to(origin, (n, 3)).copy()
    else:
        tri = blades[rng.integers(0, len(blades), n)]
        b = rng.dirichlet([1, 1, 1], n)
        pos = np.einsum("nk,nkc->nc", b, tri)
    pos = pos.astype(F32)
    do = R.unit(rng.normal(size=(n, 3)))
    m = RESPONSE_N
    fam = np.array([G_EDGE_X, G_EDGE_Y, G_SENSOR, G_SENSOR, G_CORNER, G_Z])[np.arange(m) % 6]
    step = STEPS[(np.arange(m) // 6) % len(STEPS)]
    eps = float(R.ulp32(max(W, H)))
    X, Y = rng.uniform(0, W, m), rng.uniform(0, H, m)
    axis, value = np.zeros(m, np.int64), np.zeros(m)
    ex, ey = fam == G_EDGE_X, fam == G_EDGE_Y
    value[ex] = rng.integers(1, W, ex.sum()) if W > 1 else rng.choice([0, W], ex.sum())       # a 1-pixel frame has no interior edge: its sensor edges
    value[ey] = rng.integers(1, H, ey.sum()) if H > 1 else rng.choice([0, H], ey.sum())
    axis[ey] = 1
    se = np.nonzero(fam == G_SENSOR)[0]
    which = np.arange(len(se)) % 4                                        # left, right (the last pixel's far edge), bottom, top
    axis[se], value[se] = which // 2, np.where(which % 2 == 0, 0, np.where(which // 2 == 0, W, H))
    co = fam == G_CORNER
    far = rng.random(m) < 0.5
    value[co] = np.where(far[co], W, 0)
    X = np.where(axis == 0, value + step * eps, X)
    Y = np.where(axis == 1, value + step * eps, Y)
    Y = np.where(co, np.where(far, H, 0) + step * eps, Y)                 # both coordinates on the same side: inside or outside together
    s3 = np.stack([(X / W - 0.5) * sw, (Y / H - 0.5) * sh, np.full(m, sd)], 1)
    Rinv = np.linalg.inv(g)
    ap = (pos[m:].astype(np.float64) - origin) @ Rinv.T
    local = R.unit(-s3) if kind == 1 else R.unit(-fd / sd * s3 - ap)
    z = fam == G_Z
    ang = rng.uniform(0, 2 * np.pi, m)
    flat = np.stack([np.cos(ang), np.sin(ang), step * 2.0 ** -24], 1)
    local = np.where(z[:, None], flat, local)
    axis[z], value[z] = 2, 0.0
    do[m:] = local @ g.T
    outside = np.zeros(n, bool)
    outside[m:] = z & (step == 0) & (kind == 1)                           # the pinhole with local z = 0: the reference converts a NaN or an infinity to an integer
    return pos, do.astype(F32), np.arange(n) >= m, np.concatenate([np.zeros(m, np.int64), fam]), (np.concatenate([np.zeros(m, np.int64), axis]), np.concatenate([np.zeros(m), value])), outside


def response_errors(ref, W, H, reached, pixel, value, thin):
    """over: how far (ulp of the frame's larger side, in pixels) the binary64 image point lies from where the answer puts it -- outside the
    answer's pixel, or inside the sensor by that much when the answer is "not reached"; value: ulp of the binary64 value (reached by both)."""
    reached = np.asarray(reached).astype(bool)
    cell = np.stack([np.asarray(pixel, np.int64) % W, np.asarray(pixel, np.int64) // W], 1).astype(np.float64)
    pix, size = ref["pixel"], np.array([W, H], np.float64)
    with np.errstate(all="ignore"):
        out_of_cell = np.maximum(np.maximum(cell - pix, pix - (cell + 1)), 0.0).max(1)
        depth = np.minimum(pix, size - pix).min(1)                        # how far inside the sensor
        over = np.where(reached, out_of_cell, np.where(ref["reached"], depth, 0.0))
        over = np.where(np.isnan(over), np.inf, over) / R.ulp32(max(W, H))
        if thin:                                                          # a response to a ray from behind: by how much (ulp of 1) its local z is not negative
            over = np.maximum(over, np.where(reached & (ref["z"] >= 0), ref["z"] / 2.0 ** -23, 0.0))
        both = reached & ref["reached"]
        e_v = np.where(both, np.abs(np.asarray(value, np.float64) - ref["value"]) / R.ulp32(ref["value"]), 0.0)
    return dict(over=over, value=np.where(np.isnan(e_v), np.inf, e_v))


def response_well(ref, W, H, bounds, thin):
    """Rays farther than the margin from every pixel edge, and (thin lens) with a local z farther than the margin from 0."""
    margin = R.MARGIN_FACTOR * bounds["pixel"]
    return (ref["edge"] > margin * R.ulp32(max(W, H))) & ((np.abs(ref["z"]) > margin * 2.0 ** -23) | (not thin))


def eye_weight_reference(osc, cam, W, H, eye):
    """The eye ray's weight in binary64 (thin lens): the lens response's value for that ray x 1 / p_area / pdf_dir, p_area = 1 / the
    aperture's area, pdf_dir = pixels per sensor area x sensor_distance^2 / z^4 (z: the local z of the direction)."""
    import oracle_binding as O
    kind, origin, g, fd, sd, blades = camera_geometry(osc, cam)
    ref = response_reference(osc, cam, W, H, eye[:, :3], eye[:, 3:6])
    s = O.sensor(W, H)
    area = sum(R.surface_area(R.TRIANGLE, b.reshape(9)) for b in blades)
    pdf_dir = W * H / (float(s.scene_width) * float(s.scene_height)) * sd * sd / ref["z"] ** 4
    return ref, area / pdf_dir


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


def measure_light(shares):
    """Per light kind: the oracle's worst origin residual, origin, dir and weight error (ulp) over the well-conditioned items of every light
    set, iterated until the bounds and the margins they imply reproduce themselves."""
    import oracle_binding as O
    runs = []
    for name, scene, states, aimed, fam in light_sets():
        table = light_scene_table(scene)[0]
        ref = R.light_ray(table, states)
        o, d, w, obj, used = oracle_light(O.Scene.create(**scene), states)
        runs.append((name, table, ref, light_errors(table, ref, o, d, w), used == ref["draws"], aimed))
    cur = {k: {q: 2.0 for q in LIGHT_QUANTITIES} for k in R.KIND_NAMES}
    for _ in range(8):
        b = {k: {q: R.BOUND_FACTOR * max(v, FLOOR_ULP) for q, v in qs.items()} for k, qs in cur.items()}
        worst = {k: {q: 0.0 for q in LIGHT_QUANTITIES} for k in R.KIND_NAMES}
        for name, table, ref, e, same_draws, aimed in runs:
            well = (ref["cond"] > light_margin(b, table)) & same_draws
            shares["light / " + name] = float((~well[~aimed]).mean())
            kind = table["kind"][ref["light"]]
            for k in set(int(x) for x in table["kind"]):
                s = well & (kind == k)
                if s.any():
                    for q in LIGHT_QUANTITIES:
                        worst[R.KIND_NAMES[k]][q] = max(worst[R.KIND_NAMES[k]][q], float(e[q][s].max()))
        if worst == cur:
            break
        cur = worst
    return cur


def measure_response(shares):
    """Per camera: how far (ulp of the frame's larger side, in pixels) the oracle's response lies from the binary64 image point, over every
    item inside the contract; the value's worst error on the items the margin of that calls well-conditioned; and (thin lens) the worst
    error of the eye rays' weight against the binary64 response x 1 / p_area / pdf_dir."""
    import oracle_binding as O
    out = {}
    for cam in CAMERAS:
        osc = O.Scene.create(**camera_scene(cam))
        thin = CAMERAS[cam]["n_blades"] > 0
        runs = []
        for W, H in FRAMES:
            pos, do, aimed, fam, _, outside = response_items(cam, W, H)
            ref = response_reference(osc, cam, W, H, pos, do)
            runs.append((W, H, ref, response_errors(ref, W, H, *osc.lens_responses(W, H, pos, do, math=O.MATH_GLIBC), thin), aimed, outside))
        worst = {"pixel": max(float(e["over"][~outside].max()) for _, _, _, e, _, outside in runs), "value": 0.0}
        b = {"pixel": R.BOUND_FACTOR * max(worst["pixel"], FLOOR_ULP)}
        for W, H, ref, e, aimed, outside in runs:
            well = response_well(ref, W, H, b, thin) & ~outside
            shares[f"response / {cam} {W}x{H}"] = float((~well[~aimed]).mean())
            worst["value"] = max(worst["value"], float(e["value"][well].max()))
        if thin:
            worst["eye_weight"] = 0.0
            for W, H in FRAMES:
                eye = oracle_eye(osc, W, H)
                ref, k = eye_weight_reference(osc, cam, W, H, eye)
                worst["eye_weight"] = max(worst["eye_weight"], float((np.abs(ref["value"] * k - eye[:, 6]) / R.ulp32(eye[:, 6])).max()))
        out[cam] = worst
    return out


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
    measured["light"], measured["response"] = measure_light(shares), measure_response(shares)
    doc = {"_": "Largest error of the oracle against tests/f64_reference.py on the inputs of tests/f64_inputs.py, in ulp (python tests/f64_reference.py --measure). "
                "Data only: the tests use 4 x these as bounds and 4 x the bounds as ill-conditioning margins.",
           "measured_ulp": measured, "ill_conditioned_share_of_random_half": shares}
    print(json.dumps(doc, indent=1))
    if write:
        BOUNDS_FILE.write_text(json.dumps(doc, indent=1) + "\n")
    return doc

"""The photon map of include/amber_hip.h (amber_hip_pm_build / amber_hip_pm_gather), restated in numpy to the letter: every operation binary32 and
rounded alone (numpy float32 arrays and scalars; no Python float takes part), the grid with its doubling rule, the visit order, the selection of
the k nearest with ties decided by visit order, the sum in visit order, SymmetricBSDF of the two diffuse materials, the kernel normalisation.
Phong's power is the host's powf through ctypes -- the function the device's Pow restates (dev_math.h).

Next to it, what the restatement is itself checked against (test_photon_map_reference_cpu.py): a brute force over ALL photons in binary64 that gives
the set semantics (the k nearest within the radius), with the cases in which binary32 may legitimately decide otherwise classified; and a binary32
brute force of the in-radius count, which the cell range must lose nothing of."""
import ctypes
import ctypes.util

import numpy as np

F = np.float32
PI = F(3.14159274)
QUERY = np.dtype([("pos", np.float32, (3,)), ("radius", np.float32), ("normal", np.float32, (3,)), ("object", np.int32),
                  ("dir_out", np.float32, (3,)), ("pad0", np.uint32), ("weight", np.float32, (3,)), ("pad1", np.uint32)])        # AmberGatherQuery
RESULT = np.dtype([("rgb", np.float32, (3,)), ("n_used", np.uint32), ("r2_used", np.float32), ("n_in_radius", np.uint32), ("pad", np.uint32, (2,))])   # AmberGatherResult
MAX_DIM, MAX_CELLS = 1024, 1 << 22
MAT_LAMBERTIAN, MAT_PHONG = 0, 1

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]


def powf(x, y):
    return np.array([_libm.powf(float(v), float(y)) for v in np.asarray(x, F).reshape(-1)], F)


def _ordered(x):
    """float32 -> uint32, order-preserving, -0 below +0 (the key of the build's bounds reduction)"""
    b = np.ascontiguousarray(x, F).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def _ordered_back(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(F)


def materials_of(hs):
    """Per OBJECT of a HostScene: (kind, rho (n, 3), param) -- what the gather reads through objects[object].material."""
    objs, mats, _ = hs.flatten()
    mi = np.array([o.material for o in objs], np.int64)
    kind = np.array([m.kind for m in mats], np.uint32)[mi]
    rho = np.array([[m.rho[0], m.rho[1], m.rho[2]] for m in mats], F)[mi]
    param = np.array([m.param for m in mats], F)[mi]
    return kind, rho, param


class Map:
    """info: AmberPhotonMapInfo without build_ms.  order: input index of every kept photon in cell order; start: cells + 1."""

    def __init__(self, photons, cell_size):
        pos = np.ascontiguousarray(photons["pos"], F).reshape(-1, 3)
        n = len(pos)
        kept = np.flatnonzero(np.isfinite(pos).all(axis=1))
        self.info = dict(n_photons=n, n_dropped=n - len(kept), dims=(0, 0, 0), n_doublings=0, cell_size=float(F(cell_size)), lo=(0.0, 0.0, 0.0), hi=(0.0, 0.0, 0.0),
                         max_cell_count=0)
        self.empty = len(kept) == 0
        if self.empty:
            return
        okey = _ordered(pos[kept])
        self.lo, self.hi = _ordered_back(okey.min(axis=0)), _ordered_back(okey.max(axis=0))
        c, doublings = F(cell_size), 0
        with np.errstate(over="ignore", invalid="ignore"):
            while True:
                inv = F(1) / c
                e = (self.hi - self.lo) * inv
                below = bool((e < F(2147483648.0)).all())
                dims = [int(np.floor(v)) + 1 for v in e] if below else None
                if below and max(dims) <= MAX_DIM and dims[0] * dims[1] * dims[2] <= MAX_CELLS:
                    break
                c = c * F(2)
                doublings += 1
                if not c < F(np.inf):
                    raise ValueError("the extent of the photons overflows binary32")
        self.c, self.inv, self.dims = c, inv, dims
        cf = np.floor((pos[kept] - self.lo) * inv).astype(np.int64)
        assert (cf >= 0).all() and (cf < np.array(dims)).all()                  # inside the grid by construction
        cell = (cf[:, 2] * dims[1] + cf[:, 1]) * dims[0] + cf[:, 0]
        by_cell = np.argsort(cell, kind="stable")
        self.order = kept[by_cell]
        self.start = np.searchsorted(cell[by_cell], np.arange(dims[0] * dims[1] * dims[2] + 1), side="left")
        self.pos = pos[self.order]
        self.dir_out = np.ascontiguousarray(photons["dir_out"], F).reshape(-1, 3)[self.order]
        self.weight = np.ascontiguousarray(photons["weight"], F).reshape(-1, 3)[self.order]
        self.info.update(dims=tuple(dims), n_doublings=doublings, cell_size=float(c), lo=tuple(float(v) for v in self.lo), hi=tuple(float(v) for v in self.hi),
                         max_cell_count=int(np.diff(self.start).max()))

    def cellf(self, x, a):
        return np.floor((x - self.lo[a]) * self.inv)

    def candidates(self, p, radius):
        """Positions in cell order of the photons a query visits, in visit order (iz, iy, ix ascending; a row of cells is one run)."""
        c0, c1 = [], []
        with np.errstate(over="ignore"):
            for a in range(3):
                top = F(self.dims[a] - 1)
                flo, fhi = self.cellf(p[a] - radius, a), self.cellf(p[a] + radius, a)
                if fhi < F(0) or flo > top:
                    return np.zeros(0, np.int64)
                c0.append(int(min(flo, top)) if flo > F(0) else 0)
                c1.append(int(max(fhi, F(0))) if fhi < top else self.dims[a] - 1)
        runs = []
        for iz in range(c0[2], c1[2] + 1):
            for iy in range(c0[1], c1[1] + 1):
                row = (iz * self.dims[1] + iy) * self.dims[0]
                runs.append(np.arange(self.start[row + c0[0]], self.start[row + c1[0] + 1]))
        return np.concatenate(runs) if runs else np.zeros(0, np.int64)


def dot3(u, v):
    """Dot (vector3.h): (x + y) + z, each product and sum rounded; u, v broadcast over rows"""
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def symmetric_bsdf(kind, param, normal, dir_out, dir_in):
    """fs for one (normal, dir_out) against the rows of dir_in (material_lambertian.cc:35-49, material_phong.cc:40-61); other kinds: 0"""
    dir_in = np.ascontiguousarray(dir_in, F).reshape(-1, 3)
    fs = np.zeros(len(dir_in), F)
    if kind not in (MAT_LAMBERTIAN, MAT_PHONG) or len(dir_in) == 0:
        return fs
    with np.errstate(over="ignore", invalid="ignore"):
        cos_o, cos_i = dot3(dir_out, normal), dot3(dir_in, normal)
        lit = ~(cos_o * cos_i <= F(0))
        if kind == MAT_LAMBERTIAN:
            fs[lit] = F(1) / PI
            return fs
        refl = (F(2) * cos_i)[:, None] * normal[None, :] - dir_in
        d = dot3(refl, dir_out[None, :])
        cos_alpha = np.where(F(0) < d, d, F(0)).astype(F)
        fs[lit] = (((param + F(2)) / (F(2) * PI)) * powf(cos_alpha[lit], param)).astype(F)
    return fs


def gather_one(m, q, k, raw, materials):
    """(rgb, n_used, r2_used, n_in_radius, used): the result fields for query record q, and the INPUT indices of the photons used, in visit order."""
    none = np.zeros(0, np.int64)
    zero = (np.zeros(3, F), 0, F(0), 0, none)
    kind, rho, param = materials
    p, radius, obj = q["pos"].astype(F), F(q["radius"]), int(q["object"])
    if m.empty or not np.isfinite(p).all() or not (np.isfinite(radius) and radius > F(0)) or not 0 <= obj < len(kind):
        return zero
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        r2 = radius * radius
        cand = m.candidates(p, radius)
        d = m.pos[cand] - p[None, :]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        inr = d2 < r2
        n_in = int(inr.sum())
        cand, d2 = cand[inr], d2[inr]
        if k == 0 or n_in <= k:
            used, n_used, r2_used = cand, n_in, r2
        else:
            T = np.partition(d2, k - 1)[k - 1]
            less, tie = d2 < T, d2 == T
            used = cand[less | (tie & (np.cumsum(tie) <= k - int(less.sum())))]
            n_used, r2_used = k, T
        assert len(used) == n_used
        fs = symmetric_bsdf(int(kind[obj]), param[obj], q["normal"].astype(F), q["dir_out"].astype(F), m.dir_out[used])
        terms = m.weight[used] * (rho[obj][None, :] * fs[:, None])
        S = np.cumsum(np.vstack([np.zeros((1, 3), F), terms.astype(F)]), axis=0, dtype=F)[-1]        # sequential, from +0
        if raw:
            rgb = S
        else:
            kern = F(1) / ((PI * radius) * radius)
            rgb = (S * kern) * q["weight"].astype(F)
    return rgb.astype(F), n_used, F(r2_used), n_in, m.order[used]


def gather(m, queries, k, raw, materials):
    out = np.zeros(len(queries), RESULT)
    for i, q in enumerate(queries):
        out["rgb"][i], out["n_used"][i], out["r2_used"][i], out["n_in_radius"][i], _ = gather_one(m, q, k, raw, materials)
    return out


# ---- what the restatement is checked against -------------------------------------------------------------------------------------------------------
def brute_count_f32(photons, q):
    """n_in_radius over ALL finite photons, the contract's d2 and test in binary32"""
    pos = np.ascontiguousarray(photons["pos"], F).reshape(-1, 3)
    pos = pos[np.isfinite(pos).all(axis=1)]
    with np.errstate(over="ignore"):
        d = pos - q["pos"].astype(F)[None, :]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        return int((d2 < F(q["radius"]) * F(q["radius"])).sum())


ULP = 2.0 ** -23          # of binary32, relative


def brute_knn_f64(photons, q, k):
    """The set semantics in binary64 over all photons: (input indices of the k nearest within the radius -- all of them for k == 0 or N <= k --, N,
    fragile).  fragile: binary32 may decide otherwise and still be right -- a d2 within 4 binary32 ulp of r2, or (when k cuts) the k-th and the
    (k + 1)-th distance within 4 binary32 ulp of each other: a tie at the k-th distance at the resolution the device computes with (d2 is a sum of
    three positive products of rounded differences: its relative error is below 4 * 2^-24)."""
    pos = np.ascontiguousarray(photons["pos"], F).reshape(-1, 3).astype(np.float64)
    d2 = ((pos - q["pos"].astype(np.float64)[None, :]) ** 2).sum(axis=1)
    r2 = float(q["radius"]) ** 2
    fragile = bool((np.abs(d2 - r2) <= 4 * ULP * r2).any())
    inside = np.flatnonzero(d2 < r2)
    if k == 0 or len(inside) <= k:
        return inside, len(inside), fragile
    by_distance = inside[np.argsort(d2[inside], kind="stable")]
    dk, dk1 = d2[by_distance[k - 1]], d2[by_distance[k]]
    fragile = fragile or dk1 - dk <= 4 * ULP * dk
    return np.sort(by_distance[:k]), len(inside), fragile

"""A numpy reference of the child boxes of engine BVH's tree, and a validator that holds a dumped tree to it from the OTHER side.

test_device_build.validate_tree proves a tree conservative: every box contains what is beneath it.  Every parity test rests on that, and none of
them can see boxes that are too LARGE -- the answer of engine BVH does not depend on its tree.  tree_tightness() closes that side: for every
(node, side) it forms the box the builder was supposed to quantise -- the binary32 union of the widened boxes of all leaf slots beneath the child,
padded by PadBox -- and asserts that every stored plane is within K representable binary16 values of it.

The bound follows from what tests/cpp proves: PlaneWord (host builder) stores the tightest representable value (plane_word_check.cpp), PlaneWordOutward
(device build, refit) at most one value further out (plane_word_outward_check.cpp, kMaxStepsLooser = 1).  So a stored plane moved K values INWARD
-- K = 1 for host-built trees, K = 2 for device-built, rebuilt and refitted ones -- is no longer outside the reference box.

Everything here is numpy with the roundings of bvh_build.h restated (binary64 where the C++ computes in double, one rounding where it narrows,
binary32 operations where it works in float); nothing of it calls the kernels or the host builder.
"""
import numpy as np

F32 = np.float32
EPS = 5.9604644775390625e-08
K_MAX_DEPTH = 30                                 # bvh_build.h: kMaxDepth
K_HOST, K_DEVICE = 1, 2                          # representable values a stored plane may lie outside the reference box (see above)

# The allowance of the comparison, in binary32 ulps of max(|gmin|, |reference plane|).  It covers nothing but last-bit differences between this
# restatement and the C++ (libm's hypot / sqrt, one narrowing), and PlaneWord's own guard of 2^-50 of its operands -- near the centre of the grid
# binary16 values are finer than a binary32 ulp of the coordinate, so a one-bit difference in a box is many representable values there.
# MEASURED on the host-built trees (K = 1) of every scene of tests/test_tree_tightness.py -- scenes A, and B = moved(A, 101), C = moved(A, 202) --
# as the smallest allowance under which all of them pass: 0.0 ulps (every plane of every host tree is within one representable value of the
# restated box, exactly: the restatement reproduces the host builder's boxes bit for bit, and no plane fell inside the guard).
# CHOSEN: twice the measured value = 0.0 ulps.  Never tuned on device-built or refitted trees.
ALLOWANCE_ULPS = 0.0

_MAG_MIN, _MAG_MAX = 0x0400, 0x3c01              # binary16 magnitudes 2^-14 ... 1 + 2^-10: what a plane word may hold besides zero
RANK_MAX = _MAG_MAX - _MAG_MIN + 1


# ---- object boxes -----------------------------------------------------------------------------------------------------------------------
def widened_object_boxes(arr):
    """bvh_build.h's ObjectBox of every flattened record, widened as BuildBvh / db_bounds_wide widen it (sphere slack 16 eps D^2, needle reach D with
    D the diagonal of the geometric bounds), NOT padded: (mn, mx), (n, 3) binary32."""
    kind, p = arr["kind"], arr["p"]
    a = p[:, 0:3]
    tri, sph, dsk, cyl = kind == 0, kind == 1, kind == 2, kind == 3
    e1 = np.where(tri[:, None], p[:, 3:6] - a, p[:, 3:6]).astype(F32)
    e2 = (p[:, 6:9] - a).astype(F32)
    radius = np.where(sph, p[:, 3], p[:, 6]).astype(F32)
    height = p[:, 7]

    def boxes(slack2, reach):
        mn, mx = np.empty_like(a), np.empty_like(a)
        v1, v2 = (a + e1).astype(F32), (a + e2).astype(F32)
        tmn, tmx = np.minimum(a, np.minimum(v1, v2)), np.maximum(a, np.maximum(v1, v2))
        if reach > 0:
            d1, d2_, d3 = e1.astype(np.float64), e2.astype(np.float64), e2.astype(np.float64) - e1.astype(np.float64)
            l = np.stack([(d1 * d1).sum(1), (d2_ * d2_).sum(1), (d3 * d3).sum(1)], 1)
            emax, emin = np.sqrt(l.max(1)), np.sqrt(l.min(1))
            with np.errstate(divide="ignore", invalid="ignore"):
                m = np.minimum(reach, 36.0 * EPS * reach * emax / emin)
            ok = (emin > 0) & np.isfinite(emax)
            tmn = np.where(ok[:, None], (tmn.astype(np.float64) - m[:, None]).astype(F32), tmn)
            tmx = np.where(ok[:, None], (tmx.astype(np.float64) + m[:, None]).astype(F32), tmx)
        mn[tri], mx[tri] = tmn[tri], tmx[tri]
        r = (np.sqrt(radius.astype(np.float64) ** 2 + slack2) * 1.000001).astype(F32)
        mn[sph], mx[sph] = (a - r[:, None]).astype(F32)[sph], (a + r[:, None]).astype(F32)[sph]
        rd = np.abs(radius.astype(np.float64)) * 1.000001
        nu = np.sqrt((e1.astype(np.float64) ** 2).sum(1))
        with np.errstate(divide="ignore", invalid="ignore"):
            axial = np.where(nu > 1e-30, np.abs(height.astype(np.float64)) / nu, 1e30)
        rc = np.minimum(1e30, np.hypot(radius.astype(np.float64), axial) * 1.000001)
        for sel, rr in ((dsk, rd), (cyl, rc)):
            mn[sel], mx[sel] = (a.astype(np.float64) - rr[:, None]).astype(F32)[sel], (a.astype(np.float64) + rr[:, None]).astype(F32)[sel]
        return mn, mx

    mn, mx = boxes(0.0, 0.0)
    d2 = float(((np.nanmax(mx, 0).astype(np.float64) - np.nanmin(mn, 0).astype(np.float64)) ** 2).sum())
    return boxes(16.0 * EPS * d2, np.sqrt(d2))


def scene_extent(mn, mx):
    """The extent PadBox is called with: the largest side, in binary32, of the bounds of all widened boxes.  BuildBvh (host trees: Shared::extent) and
    GridOfBounds (device-built, rebuilt and refitted trees: Grid::extent) compute it by this one formula, from bounds that skip NaN as Box::grow does."""
    return F32((np.nanmax(mx, 0) - np.nanmin(mn, 0)).astype(F32).max())


def pad_boxes(mn, mx, extent):
    """bvh_build.h's PadBox in binary32, of boxes of any leading shape (..., 3)"""
    mn, mx, extent = np.asarray(mn, F32), np.asarray(mx, F32), F32(extent)
    m = np.maximum(np.abs(mn), np.abs(mx))
    pad = (F32(1.52587890625e-05) * (extent + m).astype(F32)).astype(F32) + F32(1e-30)
    return (mn - pad).astype(F32), (mx + pad).astype(F32)


# ---- plane words ------------------------------------------------------------------------------------------------------------------------
def _rank(half):
    """position of a stored binary16 pattern among the representable values ... -2^-14, 0, 2^-14, next, ... (0 for zero)"""
    half = np.asarray(half).astype(np.int64)
    mag = half & 0x7fff
    assert (((mag == 0) | (mag >= _MAG_MIN)) & (mag <= _MAG_MAX)).all(), "a plane word holds a denormal, or a value beyond 1 + 2^-10"
    r = np.where(mag == 0, 0, mag - (_MAG_MIN - 1))
    return np.where((half & 0x8000) != 0, -r, r)


def _half(rank):
    rank = np.clip(np.asarray(rank, np.int64), -RANK_MAX, RANK_MAX)
    mag = np.where(rank == 0, 0, np.abs(rank) + (_MAG_MIN - 1))
    return (mag | np.where(rank < 0, 0x8000, 0)).astype(np.uint16)


def _value(rank):
    return _half(rank).view(np.float16).astype(np.float64)


def step_half(half, k):
    """the binary16 pattern k representable values above (k < 0: below) the stored pattern `half` -- for tests that corrupt a dump"""
    return _half(_rank(half) + k)


def plane_ranks(dump):
    """(lo, hi): (n, 2, 3) int64 ranks of the min / max plane values of the left / right child box of every node"""
    w = dump["nodes"][:, :6].reshape(-1, 2, 3)
    return _rank(w & 0xffff), _rank(w >> 16)


def decoded_planes(dump, lo_rank=None, hi_rank=None):
    """(lo, hi): (n, 2, 3) binary64 planes gmin + value * step (the product is exact: step is binary32, the value has 11 bits; the sum rounds once)"""
    if lo_rank is None:
        lo_rank, hi_rank = plane_ranks(dump)
    g, s = dump["gmin"].astype(np.float64), dump["step"].astype(np.float64)
    return g + _value(lo_rank) * s, g + _value(hi_rank) * s


# ---- the reference boxes ----------------------------------------------------------------------------------------------------------------
def tree_levels(dump):
    """the nodes of every level, the root's first; asserts a tree (every node reached once) no deeper than the traversal's limit"""
    child = dump["nodes"][:, 6:8].view(np.int32)
    n = len(child)
    assert dump["root"] == 0
    seen = np.zeros(n, bool)
    levels, frontier = [], np.array([0], np.int64)
    while len(frontier):
        assert len(levels) < K_MAX_DEPTH and not seen[frontier].any() and len(np.unique(frontier)) == len(frontier)
        seen[frontier] = True
        levels.append(frontier)
        kids = child[frontier].ravel()
        frontier = kids[kids >= 0].astype(np.int64)
        assert (frontier < n).all()
    assert seen.all()
    return levels


def reference_child_boxes(dump, wmn, wmx):
    """For every (node, side): the union, by binary32 min / max, of the widened boxes (wmn, wmx) of all leaf slots beneath that child -- NaN bounds
    skipped as Box::grow skips them.  Bottom-up over the dumped topology, a level at a time.  (n, 2, 3) binary32 each; not padded.  min / max are
    exact, so the union does not depend on the order in which a builder formed it."""
    child = dump["nodes"][:, 6:8].view(np.int32)
    prims = dump["prims"].astype(np.int64)
    n, n_obj = len(child), len(prims)
    rmn, rmx = np.full((n, 2, 3), F32(3.0e38)), np.full((n, 2, 3), F32(-3.0e38))       # Box::reset
    for level in reversed(tree_levels(dump)):
        for side in (0, 1):
            ref = child[level, side]
            leaf = ref < 0
            r = -(ref[leaf].astype(np.int64) + 1)
            first, count, nd = r >> 4, r & 3, level[leaf]
            assert ((count >= 1) & (first + count <= n_obj)).all()
            for k in range(3):
                sel = count > k
                obj = prims[(first + k)[sel]]
                rmn[nd[sel], side] = np.fmin(rmn[nd[sel], side], wmn[obj])
                rmx[nd[sel], side] = np.fmax(rmx[nd[sel], side], wmx[obj])
            nd, kid = level[~leaf], ref[~leaf].astype(np.int64)                           # (the kids are a level further down: done)
            rmn[nd, side] = np.fmin(rmn[kid, 0], rmn[kid, 1])
            rmx[nd, side] = np.fmax(rmx[kid, 0], rmx[kid, 1])
    return rmn, rmx


# ---- the validator ----------------------------------------------------------------------------------------------------------------------
MAX_LOOSENESS = 64                               # looseness is searched this far; a plane further out reports MAX_LOOSENESS + 1


def tree_tightness(dump, arr, k, allowance_ulps=ALLOWANCE_ULPS, label="", boxes=None):
    """Asserts that every plane of the dumped tree, moved k representable values inward, lies inside the reference box of its child or within the
    allowance of it.  `arr`: the flattened object records; boxes: widened_object_boxes(arr) when the caller has them already.
    Returns dict(planes, looseness, needed_ulps):
    planes       planes judged: 6 * 2 * n_nodes, asserted (every reference box of the scenes in use is finite)
    looseness    the largest, over all planes, number of representable values a plane has to move inward until it is no longer outside its
                 reference box (a tight host plane: 1; the tree is accepted iff looseness <= k)
    needed_ulps  the smallest allowance, in binary32 ulps of max(|gmin|, |reference plane|), under which this tree passes at k"""
    n = len(dump["nodes"])
    if n == 0:
        return dict(planes=0, looseness=0, needed_ulps=0.0)
    wmn, wmx = boxes if boxes is not None else widened_object_boxes(arr)
    assert len(dump["prims"]) == len(arr) == len(wmn)
    rmn, rmx = reference_child_boxes(dump, wmn, wmx)
    assert (np.abs(rmn) < 3.0e38).all() and (np.abs(rmx) < 3.0e38).all() and (rmn <= rmx).all(), (label, "a reference box is empty or not finite")
    pmn, pmx = pad_boxes(rmn, rmx, scene_extent(wmn, wmx))
    g = np.abs(dump["gmin"]).astype(F32)
    ulp = np.stack([np.spacing(np.maximum(g, np.abs(pmn))), np.spacing(np.maximum(g, np.abs(pmx)))], 2).astype(np.float64)
    lo_rank, hi_rank = plane_ranks(dump)

    def deficit(j):
        """(n, 2, 2, 3), axis 2 = min planes, max planes: how far, in ulps, the stored plane moved j values inward is still OUTSIDE the reference box"""
        lo, hi = decoded_planes(dump, lo_rank + j, hi_rank - j)                           # inward: min planes up, max planes down
        return np.stack([pmn.astype(np.float64) - lo, hi - pmx.astype(np.float64)], 2) / ulp

    at_k = deficit(k)
    planes = int(np.isfinite(at_k).sum())
    assert planes == 6 * 2 * n, (label, planes, n)
    needed = float(max(0.0, at_k.max()))
    steps = np.full(at_k.shape, MAX_LOOSENESS + 1, np.int64)
    for j in range(MAX_LOOSENESS + 1):
        outside = steps > MAX_LOOSENESS
        if not outside.any():
            break
        steps[outside & (deficit(j) <= allowance_ulps)] = j
    looseness = int(steps.max())
    if looseness > k:
        node, side, which, axis = (int(x) for x in np.unravel_index(steps.argmax(), steps.shape))
        raise AssertionError(f"{label}: a box is too large: the {'max' if which else 'min'} plane of axis {axis} of node {node}, side {side}, lies {looseness}"
                             f"{'+' if looseness > MAX_LOOSENESS else ''} representable values outside its reference box (allowed: {k}); "
                             f"{int((steps > k).sum())} of {planes} planes do; the tree would pass with an allowance of {needed:.3g} ulps")
    return dict(planes=planes, looseness=looseness, needed_ulps=needed)


# ---- the quality figure of AmberUpdateInfo ------------------------------------------------------------------------------------------------
def reference_area(dump):
    """area_before / area_after of amber_hip_pt_update_objects for this dump: the sum over inner nodes of both child boxes' surface areas, divided
    by the surface area of the root (the union of the root node's two boxes), in binary64 from the decoded planes.  0 for a scene that is one leaf."""
    if len(dump["nodes"]) == 0 or dump["root"] < 0:
        return 0.0
    lo, hi = decoded_planes(dump)

    def area(lo, hi):
        e = hi - lo
        a = 2.0 * (e[..., 0] * e[..., 1] + e[..., 1] * e[..., 2] + e[..., 2] * e[..., 0])
        return np.where((e < 0).any(-1), 0.0, a)
    root = float(area(lo[0].min(0), hi[0].max(0)))
    return float(area(lo, hi).sum()) / root if root > 0 else 0.0

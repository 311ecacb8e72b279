// filter_build.h -- host-side construction of the Phase-A filter program of the two-phase closest hit
// (device side: ClosestHitTwoPhase in dev_two_phase.h).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../../include/amber_hip.h"
#include "pt_device.h"

namespace amber_filter {

using amber_dev::DevObject;
using amber_dev::DevPlane;
using amber_dev::DevSphereFilter;
using amber_dev::DevTriFilter;

// Phase-A program of the two-phase closest hit.  Everything here only has to be CONSERVATIVE: a candidate that
// the filter keeps is decided by the exact reference-arithmetic test, so these values are computed in double and
// rounded once.  Tolerances: the reference's binary32 Moeller-Trumbore has an absolute error of at most
// ~6 eps (|o - v0| + 1.5 |E|) / |cos| in world units along the triangle's plane; with eps = 2^-24 and a safety
// factor the bound used is  c / |n.d|,  c = 32 eps (scene diameter + 1.5 max edge), turned into barycentric units
// with the gradient magnitudes of the affine barycentric maps.  Coplanar triangles (all vertices within 4 eps of
// the scene diameter of the first triangle's plane) share a plane record; their distance to it joins the tolerance.
struct FilterProgram {
  std::vector<DevPlane> planes;
  std::vector<DevTriFilter> tris;
  std::vector<DevSphereFilter> spheres;
  std::vector<uint32_t> order;          // program slot -> scene object index
  uint32_t n_prog_tris = 0, always_mask = 0;
  uint32_t n_simple_planes = 0;         // the first planes of the program (an even number) form slabs: two parallel planes of one parallelogram pair each
  uint32_t n_axis_slabs[3] = {0, 0, 0}; // the first of these slabs are axis slabs (below), per axis x, y, z; they stand in the order AxisSlabOrder(0), (1), (2)
};
// The axis of the k-th axis loop of the device (dev_two_phase.h: AMBER_AXIS_FIRST)
inline int AxisSlabOrder(int k) { return (AMBER_AXIS_FIRST + k) % 3; }

// DevScene::slab_ends / DevFilterGroup::slab_ends of a program (at most 32 objects, so at most 16 slab planes: a byte each)
inline uint32_t SlabEnds(const FilterProgram& fp) {
  const uint32_t e0 = 2u * fp.n_axis_slabs[AxisSlabOrder(0)], e1 = e0 + 2u * fp.n_axis_slabs[AxisSlabOrder(1)], e2 = e1 + 2u * fp.n_axis_slabs[AxisSlabOrder(2)];
  return e0 | e1 << 8 | e2 << 16 | fp.n_simple_planes << 24;
}
// The two in-plane axes (u < v) of an axis slab of axis c: row `a` of its pair records depends on P_u alone, row `b` on P_u and P_v.
inline void AxisSlabInPlane(int c, int& u, int& v) { u = c == 0 ? 1 : 0; v = c == 2 ? 1 : 2; }
// The axis c of which a plane of ONE pair record is an axis-slab plane, judged on the binary32 values the device reads, or -1: the normal is
// +-1 in component c and +-0 elsewhere, both rows of the record have a +-0 coefficient for coordinate c, and row `a` has exactly one non-zero
// gradient coefficient, that of the first in-plane axis.  The device's axis loops leave out exactly these zero terms (dev_two_phase.h).
inline int AxisSlabClass(const DevPlane& p, const DevTriFilter& f) {
  for (int c = 0; c < 3; c++) {
    int u, v; AxisSlabInPlane(c, u, v);
    if (std::fabs(p.n[c]) == 1.0f && p.n[u] == 0.0f && p.n[v] == 0.0f)
      return (f.c[c][0] == 0.0f && f.c[c][1] == 0.0f && f.c[u][1] != 0.0f && f.c[v][1] == 0.0f) ? c : -1;
  }
  return -1;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// Flat self (AMBER_FLAT_SELF, dev_two_phase.h): the self candidate of a bounce ray that leaves an AXIS-FLAT triangle is dropped without arithmetic.
//
// CLAIM.  Let a triangle's stored binary32 record (A, E1, E2) have, for some axis c, E1_c and E2_c both +-0, and every component of A, E1 and E2
// finite with magnitude below 2^40.  Let (u, v) be what IntersectTriangle stored with a hit on it, let pos be what ResolveHit forms from them and this
// record, and let a ray of ANY direction d start at o = pos.  Then the t of this triangle in that cast -- the self trip's and the full test's are the
// same expression, Dot(Cross(o - A, E1), E2) / det, det = Dot(Cross(d, E2), E1) -- is +-0 or NaN.  The self trip clears the bit on t <= kEPS (+-0) and
// leaves a NaN to the full test, whose `!(t <= kEPS) && Closer(t)` refuses +-0 by its first half and NaN by IsFinite: the triangle can never become
// the hit, and clearing its bit beforehand leaves HitRec as it is.  Every operation below is one binary32 operation rounded to nearest (the
// translation unit is built with -ffp-contract=off; a fused form of the same products would give the same zeros).  a, b: the two other axes.
//
//  1. (u, v).  The hit passed !(u > 1 || u < 0) and the same for v: each is in [0, 1] (-0 and subnormals included) or NaN.
//  2. NaN u or v.  pos_k = (A_k + u E1_k) + v E2_k, k = x, y, z: a NaN factor makes all three components NaN, so o - A is NaN in every component of
//     every object's test, every distance of the next cast is NaN and nothing is hit at all -- with or without the bit.  From here on u, v are in [0, 1].
//  3. The zero products.  u E1_c and v E2_c are a finite number times +-0: +-0.
//  4. pos_c.  A_c + (+-0) is A_c for A_c != 0, and a zero (+0 unless both are -0) for A_c = +-0; adding the second +-0 repeats that.  pos_c has the
//     VALUE of A_c; only the sign of a zero can differ -- A_c = -0 gives pos_c = +0 unless both products are -0.
//  5. T = o - A.  T_c = pos_c - A_c is x - x = +0 for x != 0, and (+-0) - (+-0) = +-0 for the zeros.  T_a and T_b are finite:
//     |pos_k| <= |A_k| + |E1_k| + |E2_k| < 3 * 2^40 before two roundings, so |T_k| < 2^43.
//  6. Q = Cross(T, E1).  Q_a = T_b E1_c - T_c E1_b and Q_b = T_c E1_a - T_a E1_c: each product has a +-0 factor and a FINITE one, so it is +-0, and
//     a difference of zeros is +-0.  Q_c = T_a E1_b - T_b E1_a is finite: |Q_c| < 2 * 2^43 * 2^40 = 2^84.
//  7. The numerator Dot(Q, E2) = Q_x E2_x + Q_y E2_y + Q_z E2_z.  Q_a E2_a and Q_b E2_b are +-0 times finite, Q_c E2_c is finite times E2_c = +-0:
//     three zeros, whose sums are +-0.  The numerator is an exact zero of either sign.
//  8. The sign of zero never matters: +0 and -0 alike satisfy t <= kEPS, and neither is ever stored.
//  9. det.  +-0 / det is +-0 for det finite and non-zero and for det = +-inf; it is NaN for det = +-0 and for det NaN.  Both outcomes are refused (above).
// 10. The magnitude bound is what keeps every second factor in 6 and 7 finite: inf * 0 would be NaN, not zero.  With all stored components below 2^40
//     the largest intermediate is below 2^84 < 2^128, whatever u, v in [0, 1] and whatever d.  (A NaN would be refused as well; the bound lets the
//     claim, and the host test of it, say "zero".)
//
// The premise "o is ResolveHit's pos of this record" holds where PathShade (dev_shading.h) sets origin_slot after o = pos, and only there: eye rays,
// light rays and callers' rays form their origins otherwise and keep plain slots.  The mark is per record of the LDS image (prog_objects); engine
// LIST's records, the reference of the tests, are not touched.  tests/cpp/flat_self_check.hip draws the claim at random.
inline bool FlatSelfTriangle(const DevObject& o) {
  if ((o.kind & 0xffu) != AMBER_PRIM_TRIANGLE) return false;
  uint32_t a[3], e1[3], e2[3];
  std::memcpy(a, o.a, sizeof a); std::memcpy(e1, o.e1, sizeof e1); std::memcpy(e2, o.e2, sizeof e2);
  bool flat = false;
  for (int c = 0; c < 3; c++) {
    flat = flat || ((e1[c] & 0x7fffffffu) == 0u && (e2[c] & 0x7fffffffu) == 0u);                       // +-0 by the bit pattern, sign masked off
    const uint32_t below = 0x53800000u;                                                                  // 2^40: magnitudes order like their bit patterns; inf and NaN are above
    if ((a[c] & 0x7fffffffu) >= below || (e1[c] & 0x7fffffffu) >= below || (e2[c] & 0x7fffffffu) >= below) return false;
  }
  return flat;
}
// The marks of the 32-object engine's LDS image: program slots [0, n_prog_tris) are the filtered triangles; `radius` is a dword no triangle uses.
inline void MarkFlatSelf(std::vector<DevObject>& prog, uint32_t n_prog_tris) {
#if AMBER_FLAT_SELF
  const uint32_t mark = AMBER_FLAT_SELF_MARK;
  for (size_t k = 0; k < prog.size() && k < n_prog_tris && k < 32; k++)
    if (FlatSelfTriangle(prog[k])) std::memcpy(&prog[k].radius, &mark, sizeof mark);
#else
  (void)prog; (void)n_prog_tris;
#endif
}

// `center`: the filter works in coordinates relative to this point (the device subtracts it from the ray origin), so its
// affine maps see magnitudes of the order of the scene size however far the scene lies from the world origin; in
// absolute coordinates u = A.P + a0 cancels two large terms and loses the precision the tolerances assume
// (found by fuzzing with scenes offset by 1e4 of their size).
// `subset` (engine TWO_PHASE_N): the scene indices of the group the program is for, at most 32; null = the scene's first 32 objects.  Tolerances
// always derive from the bounds of ALL objects.
inline void BuildFilterProgram(const std::vector<DevObject>& objs, const float center[3], FilterProgram& fp, const std::vector<uint32_t>* subset = nullptr) {
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, e_max = 0;
  auto grow = [&](double x, double y, double z) {
    const double p[3] = {x, y, z};
    for (int c = 0; c < 3; c++) { if (p[c] < lo[c]) lo[c] = p[c]; if (p[c] > hi[c]) hi[c] = p[c]; }
  };
  auto len3 = [](const double* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
  for (const DevObject& o : objs) {
    if (o.kind == AMBER_PRIM_TRIANGLE) {
      grow(o.a[0], o.a[1], o.a[2]);
      grow(double(o.a[0]) + o.e1[0], double(o.a[1]) + o.e1[1], double(o.a[2]) + o.e1[2]);
      grow(double(o.a[0]) + o.e2[0], double(o.a[1]) + o.e2[1], double(o.a[2]) + o.e2[2]);
      const double E1[3] = {o.e1[0], o.e1[1], o.e1[2]}, E2[3] = {o.e2[0], o.e2[1], o.e2[2]};
      e_max = std::max(e_max, std::max(len3(E1), len3(E2)));
    } else {
      const double r = std::fabs(double(o.radius)) + std::fabs(double(o.height));
      grow(o.a[0] - r, o.a[1] - r, o.a[2] - r); grow(o.a[0] + r, o.a[1] + r, o.a[2] + r);
    }
  }
  const double diam = std::sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
  const double eps = 5.9604644775390625e-08;
  const double c = 32.0 * eps * (diam + 1.5 * e_max);
  // per triangle of a group: the three affine coordinate functions (of v0, v1, v2) in double, for pairing
  struct Tri { uint32_t index; double v[3][3]; double coef[3][4]; double g; };   // coef[k] = (gradient, constant) of the coordinate of vertex k
  struct Group { double n[3], d0, kt, ktol; std::vector<Tri> tris; bool flip = false, same_normal = false; };
  std::vector<Group> groups;
  std::vector<uint32_t> sphere_index, always_index;
  const size_t n_members = subset ? std::min<size_t>(subset->size(), 32) : std::min<size_t>(objs.size(), 32);
  for (size_t member = 0; member < n_members; member++) {
    const uint32_t idx = subset ? (*subset)[member] : static_cast<uint32_t>(member);
    const DevObject& o = objs[idx];
    if (o.kind == AMBER_PRIM_TRIANGLE) {
      const double v0[3] = {double(o.a[0]) - center[0], double(o.a[1]) - center[1], double(o.a[2]) - center[2]};   // centred
      const double E1[3] = {o.e1[0], o.e1[1], o.e1[2]}, E2[3] = {o.e2[0], o.e2[1], o.e2[2]};
      const double nr[3] = {E1[1] * E2[2] - E1[2] * E2[1], E1[2] * E2[0] - E1[0] * E2[2], E1[0] * E2[1] - E1[1] * E2[0]};
      const double n2 = nr[0] * nr[0] + nr[1] * nr[1] + nr[2] * nr[2];
      if (!(n2 > 1e-60) || !std::isfinite(n2)) { always_index.push_back(idx); continue; }
      const double nl = std::sqrt(n2);
      const double n[3] = {nr[0] / nl, nr[1] / nl, nr[2] / nl};
      const double d0 = n[0] * v0[0] + n[1] * v0[1] + n[2] * v0[2];
      // u = A.(P - v0), A = (E2 x nr)/|nr|^2 ; v = B.(P - v0), B = (nr x E1)/|nr|^2
      const double A[3] = {(E2[1] * nr[2] - E2[2] * nr[1]) / n2, (E2[2] * nr[0] - E2[0] * nr[2]) / n2, (E2[0] * nr[1] - E2[1] * nr[0]) / n2};
      const double B[3] = {(nr[1] * E1[2] - nr[2] * E1[1]) / n2, (nr[2] * E1[0] - nr[0] * E1[2]) / n2, (nr[0] * E1[1] - nr[1] * E1[0]) / n2};
      const double AB[3] = {A[0] + B[0], A[1] + B[1], A[2] + B[2]};
      const double g = std::max(len3(A), std::max(len3(B), len3(AB)));
      const double inv_sin = len3(E1) * len3(E2) / nl;
      // find a plane group that contains all three vertices
      const double verts[3][3] = {{v0[0], v0[1], v0[2]}, {v0[0] + E1[0], v0[1] + E1[1], v0[2] + E1[2]}, {v0[0] + E2[0], v0[1] + E2[1], v0[2] + E2[2]}};
      Group* grp = nullptr; double dist = 0;
      for (Group& gq : groups) {
        double dmax = 0;
        for (const auto& vtx : verts) dmax = std::max(dmax, std::fabs(gq.n[0] * vtx[0] + gq.n[1] * vtx[1] + gq.n[2] * vtx[2] - gq.d0));
        if (dmax <= 4.0 * eps * diam) { grp = &gq; dist = dmax; break; }
      }
      Tri t;
      t.index = idx; t.g = g;
      for (int k = 0; k < 3; k++) for (int c2 = 0; c2 < 3; c2++) t.v[k][c2] = verts[k][c2];
      const double a0 = -(A[0] * v0[0] + A[1] * v0[1] + A[2] * v0[2]), b0 = -(B[0] * v0[0] + B[1] * v0[1] + B[2] * v0[2]);
      for (int k = 0; k < 3; k++) { t.coef[1][k] = A[k]; t.coef[2][k] = B[k]; t.coef[0][k] = -(A[k] + B[k]); }
      t.coef[1][3] = a0; t.coef[2][3] = b0; t.coef[0][3] = 1.0 - a0 - b0;
      const double ktol = (c + dist) * g * 1.0001 + 1e-7;
      const double kt = 2.0 * (c + dist) * std::max(1.0, inv_sin) + 1e-7;
      if (!std::isfinite(ktol) || !std::isfinite(static_cast<float>(a0)) || !std::isfinite(static_cast<float>(b0)) || !std::isfinite(kt)) { always_index.push_back(idx); continue; }
      if (!grp) { groups.push_back(Group{{n[0], n[1], n[2]}, d0, 0.0, 0.0, {}, false, false}); grp = &groups.back(); }
      grp->kt = std::max(grp->kt, kt);
      grp->ktol = std::max(grp->ktol, ktol);
      grp->tris.push_back(t);
    } else if (o.kind == AMBER_PRIM_SPHERE) {
      DevSphereFilter f;
      std::memset(&f, 0, sizeof f);
      for (int k = 0; k < 3; k++) f.c[k] = static_cast<float>(double(o.a[k]) - center[k]);   // centred
      f.r2 = static_cast<float>(double(o.radius) * double(o.radius));
      f.ktol = 1e-5f;
      if (!std::isfinite(f.r2)) { always_index.push_back(idx); continue; }
      fp.spheres.push_back(f);
      sphere_index.push_back(idx);
    } else {
      always_index.push_back(idx);                   // disk, cylinder: always tested exactly
    }
  }
  auto record = [](const Tri& t, int row_a, int row_b) {          // rows = vertex whose coordinate function is evaluated
    DevTriFilter f;
    std::memset(&f, 0, sizeof f);
    for (int k = 0; k < 4; k++) { f.c[k][0] = static_cast<float>(t.coef[row_a][k]); f.c[k][1] = static_cast<float>(t.coef[row_b][k]); }
    return f;
  };
  // Program order.  Phase A prunes by distance ONE-SIDEDLY (ClosestHitTwoPhase): a certain hit only removes candidates
  // that are evaluated after it, so occluders should come first.  Spheres are evaluated before all planes; planes are
  // sorted by the distance of their triangles' centroid from the area-weighted centroid of all triangles -- inner
  // surfaces (the water surface, the light just under the ceiling) before the enclosing walls, the far-away aperture
  // last.  Any order is correct; this one only makes the pruning effective.
  {
    double cw[3] = {0, 0, 0}, wsum = 0;
    std::vector<double> gc(groups.size() * 3, 0.0);
    for (size_t gi = 0; gi < groups.size(); gi++) {
      double gw = 0;
      for (const Tri& t : groups[gi].tris) {
        const double e1[3] = {t.v[1][0] - t.v[0][0], t.v[1][1] - t.v[0][1], t.v[1][2] - t.v[0][2]};
        const double e2[3] = {t.v[2][0] - t.v[0][0], t.v[2][1] - t.v[0][1], t.v[2][2] - t.v[0][2]};
        const double cr[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double area = 0.5 * len3(cr);
        for (int k = 0; k < 3; k++) gc[gi * 3 + k] += area * (t.v[0][k] + t.v[1][k] + t.v[2][k]) / 3.0;
        gw += area;
      }
      for (int k = 0; k < 3; k++) { cw[k] += gc[gi * 3 + k]; if (gw > 0) gc[gi * 3 + k] /= gw; }
      wsum += gw;
    }
    if (wsum > 0) for (int k = 0; k < 3; k++) cw[k] /= wsum;
    // Parallel planes are kept adjacent (they share n.d, n.o and the reciprocal on the device): planes are classed by
    // normal direction up to sign; classes are ordered by their innermost member, members by distance.  A member whose
    // normal is the negative of its class's first normal is stored with normal and offset negated (the same plane).
    std::vector<int> cls(groups.size(), -1);
    std::vector<size_t> cls_first;
    for (size_t gi = 0; gi < groups.size(); gi++) {
      for (size_t c = 0; c < cls_first.size() && cls[gi] < 0; c++) {
        const Group& f = groups[cls_first[c]];
        const double dot = f.n[0] * groups[gi].n[0] + f.n[1] * groups[gi].n[1] + f.n[2] * groups[gi].n[2];
        const double sgn = dot < 0 ? -1.0 : 1.0;
        // The same direction only if the BINARY32 normals the device will use are identical up to sign: the member then
        // adopts the class's normal without moving its plane (its d0 was computed with its own normal; a merely nearly
        // parallel plane -- 1e-6 rad passes a 1e-12 test on the dot product -- would be tilted by that angle times the scene
        // size, which the rounding-only tolerances kt / ktol do not cover).
        bool same = true;
        for (int k = 0; k < 3; k++) same = same && static_cast<float>(groups[gi].n[k]) == static_cast<float>(sgn * f.n[k]);
        if (same) {
          cls[gi] = static_cast<int>(c);
          for (int k = 0; k < 3; k++) groups[gi].n[k] = sgn * f.n[k];
          groups[gi].flip = dot < 0;
        }
      }
      if (cls[gi] < 0) { cls[gi] = static_cast<int>(cls_first.size()); cls_first.push_back(gi); }
    }
    auto dist2 = [&](size_t gi) { double d2 = 0; for (int k = 0; k < 3; k++) d2 += (gc[gi * 3 + k] - cw[k]) * (gc[gi * 3 + k] - cw[k]); return d2; };
    std::vector<double> cls_min(cls_first.size(), 1e300);
    for (size_t gi = 0; gi < groups.size(); gi++) cls_min[cls[gi]] = std::min(cls_min[cls[gi]], dist2(gi));
    std::vector<size_t> perm(groups.size());
    for (size_t gi = 0; gi < perm.size(); gi++) perm[gi] = gi;
    std::stable_sort(perm.begin(), perm.end(), [&](size_t x, size_t y) {
      if (cls[x] != cls[y]) return cls_min[cls[x]] != cls_min[cls[y]] ? cls_min[cls[x]] < cls_min[cls[y]] : cls[x] < cls[y];
      return dist2(x) < dist2(y);
    });
    std::vector<Group> sorted;
    int prev_cls = -1;
    for (size_t gi : perm) {
      sorted.push_back(groups[gi]);
      sorted.back().same_normal = cls[gi] == prev_cls;
      prev_cls = cls[gi];
    }
    groups.swap(sorted);
  }
  std::vector<DevTriFilter> other_corner;   // per record of fp.tris: a pair's record with row `a` taken at the OTHER shared corner (a single triangle's: itself)
  for (const Group& g : groups) {
    // Parallelogram pairs: triangle j shares two corners with triangle i and its third corner is D = A + C - B
    // (B = i's unshared corner), everything up to 1e-6 of the scene diameter; the actual mismatch (corners are
    // rebuilt from binary32 edge vectors) joins the barycentric tolerance through the gradient magnitude.
    const size_t nt = g.tris.size();
    std::vector<int> partner(nt, -1), unshared(nt, -1);
    double pair_slack = 0;
    auto apart = [](const double* p, const double* r) { return std::max(std::fabs(p[0] - r[0]), std::max(std::fabs(p[1] - r[1]), std::fabs(p[2] - r[2]))); };
    for (size_t i = 0; i < nt; i++) {
      if (partner[i] >= 0) continue;
      for (size_t j = i + 1; j < nt && partner[i] < 0; j++) {
        if (partner[j] >= 0) continue;
        int match_i[3] = {-1, -1, -1}, n_shared = 0;               // match_i[k] = corner of j equal to corner k of i
        bool used_j[3] = {false, false, false};
        double err = 0;
        for (int k = 0; k < 3; k++)
          for (int l = 0; l < 3; l++)
            if (!used_j[l] && match_i[k] < 0 && apart(g.tris[i].v[k], g.tris[j].v[l]) <= 1e-6 * diam) {
              match_i[k] = l; used_j[l] = true; n_shared++;
              err = std::max(err, apart(g.tris[i].v[k], g.tris[j].v[l]));
            }
        if (n_shared != 2) continue;
        int bi = -1, dj = -1;
        for (int k = 0; k < 3; k++) if (match_i[k] < 0) bi = k;
        for (int l = 0; l < 3; l++) if (!used_j[l]) dj = l;
        double expect[3];
        for (int c2 = 0; c2 < 3; c2++) {
          expect[c2] = -g.tris[i].v[bi][c2];
          for (int k = 0; k < 3; k++) if (k != bi) expect[c2] += g.tris[i].v[k][c2];
        }
        err = std::max(err, apart(expect, g.tris[j].v[dj]));
        if (err <= 1e-6 * diam) {
          partner[i] = static_cast<int>(j); partner[j] = static_cast<int>(i); unshared[i] = bi;
          pair_slack = std::max(pair_slack, 4.0 * err * std::max(g.tris[i].g, g.tris[j].g));
        }
      }
    }
    DevPlane p;
    std::memset(&p, 0, sizeof p);
    for (int k = 0; k < 3; k++) p.n[k] = static_cast<float>(g.flip ? -g.n[k] : g.n[k]);   // the class's first normal, bit for bit
    // the pair evaluation adds two roundings of 1 - x (<= 1.2e-7 each) and the corner mismatch measured above
    p.d0 = static_cast<float>(g.flip ? -g.d0 : g.d0); p.kt = static_cast<float>(g.kt * 1.0001); p.ktol = static_cast<float>((g.ktol + 4e-7 + pair_slack) * 1.0001);
    for (size_t i = 0; i < nt; i++) {
      if (partner[i] < 0 || static_cast<size_t>(partner[i]) < i) continue;
      const int bi = unshared[i], ai = (bi + 1) % 3;
      fp.tris.push_back(record(g.tris[i], bi, ai));
      other_corner.push_back(record(g.tris[i], bi, (bi + 2) % 3));
      fp.order.push_back(g.tris[i].index); fp.order.push_back(g.tris[static_cast<size_t>(partner[i])].index);
      p.n_pairs++;
    }
    for (size_t i = 0; i < nt; i++) {
      if (partner[i] >= 0) continue;
      fp.tris.push_back(record(g.tris[i], 1, 2));                  // u, v = coordinates of v1, v2
      other_corner.push_back(fp.tris.back());
      fp.order.push_back(g.tris[i].index);
      p.n_tris++;
    }
    if (g.same_normal) p.n_tris |= 0x80000000u;
    fp.planes.push_back(p);
  }
  // Slabs first.  A plane that holds exactly one parallelogram pair and nothing else -- a wall, a floor, a rectangular
  // light -- and is followed by another such plane with the SAME stored normal forms a slab with it; the slabs go first, in
  // their relative order, and the device runs them two planes per iteration with neither inner record loops nor the
  // "same normal?" branch (ClosestHitTwoPhase: that code is bound by instruction delivery, and every scalar branch of the
  // nested loops costs about as much as four VALU instructions).  Everything else follows in the general form; "same
  // normal as the previous plane" is re-derived for the new order.
  // Axis slabs.  A slab both of whose planes are axis-slab planes of axis c (AxisSlabClass) is stored in a reduced form that the device
  // evaluates without the terms that are zero: the normal as +e_c (a plane of normal -e_c with n and d0 negated: the same plane, and the device
  // uses only |1 / n.d|, the distance and |n.d|), and row `a` of the pair record at that shared corner whose coordinate depends on the FIRST
  // in-plane axis (the pair test is symmetric in the two shared corners: both minima are taken over the same three quantities).  The form is
  // chosen by WHERE a slab stands -- the slabs of one axis, of the next, of the third (AxisSlabOrder), the other slabs, then the general planes -- not by a branch per record; the
  // records keep their layout, and the general slab loop computes the same values from them (the dropped terms are exact zeros).
  {
    struct Span { size_t rec, slot; };
    std::vector<Span> span(fp.planes.size());
    { size_t rec = 0, slot = 0;
      for (size_t i = 0; i < fp.planes.size(); i++) {
        span[i] = Span{rec, slot};
        const uint32_t nt = fp.planes[i].n_tris & 0x7fffffffu, np = fp.planes[i].n_pairs;
        rec += np + nt; slot += 2 * np + nt;
      } }
    auto simple = [&](size_t i) { return fp.planes[i].n_pairs == 1 && (fp.planes[i].n_tris & 0x7fffffffu) == 0; };
    enum { kSlabOther = 3, kGeneral = 4 };                          // 0, 1, 2: axis slab of that axis
    std::vector<int> kind(fp.planes.size(), kGeneral);
    for (size_t i = 0; i + 1 < fp.planes.size(); i++) {
      if (!(simple(i) && simple(i + 1) && std::memcmp(fp.planes[i].n, fp.planes[i + 1].n, sizeof fp.planes[i].n) == 0)) continue;
      int axis[2]; bool other[2];
      for (size_t k = 0; k < 2; k++) {
        axis[k] = AxisSlabClass(fp.planes[i + k], fp.tris[span[i + k].rec]);
        other[k] = axis[k] < 0;                                      // row `a` at the other shared corner?
        if (other[k]) axis[k] = AxisSlabClass(fp.planes[i + k], other_corner[span[i + k].rec]);
      }
      if (axis[0] >= 0 && axis[0] == axis[1]) {
        for (size_t k = 0; k < 2; k++) {
          DevPlane& q = fp.planes[i + k];
          if (other[k]) fp.tris[span[i + k].rec] = other_corner[span[i + k].rec];
          if (q.n[axis[0]] < 0.0f) q.d0 = -q.d0;
          for (int c2 = 0; c2 < 3; c2++) q.n[c2] = c2 == axis[0] ? 1.0f : 0.0f;
        }
        kind[i] = kind[i + 1] = axis[0];
      } else kind[i] = kind[i + 1] = kSlabOther;
      i++;
    }
    std::vector<DevPlane> planes; std::vector<DevTriFilter> tris; std::vector<uint32_t> order;
    for (int pass = 0; pass <= kGeneral; pass++)
      for (size_t i = 0; i < fp.planes.size(); i++) {
        if (kind[i] != (pass < kSlabOther ? AxisSlabOrder(pass) : pass)) continue;
        DevPlane q = fp.planes[i];
        const uint32_t nt = q.n_tris & 0x7fffffffu, np = q.n_pairs;
        q.n_tris = nt;
        if (!planes.empty() && std::memcmp(planes.back().n, q.n, sizeof q.n) == 0) q.n_tris |= 0x80000000u;
        planes.push_back(q);
        for (uint32_t k = 0; k < np + nt; k++) tris.push_back(fp.tris[span[i].rec + k]);
        for (uint32_t k = 0; k < 2 * np + nt; k++) order.push_back(fp.order[span[i].slot + k]);
        if (pass < kGeneral) fp.n_simple_planes++;
        if (pass < kSlabOther && (fp.n_simple_planes & 1u) == 0u) fp.n_axis_slabs[AxisSlabOrder(pass)]++;
      }
    fp.planes.swap(planes); fp.tris.swap(tris); fp.order.swap(order);
  }
  fp.n_prog_tris = static_cast<uint32_t>(fp.order.size());
  fp.order.insert(fp.order.end(), sphere_index.begin(), sphere_index.end());
  for (uint32_t idx : always_index) { fp.always_mask |= 1u << fp.order.size(); fp.order.push_back(idx); }
}

}  // namespace amber_filter

// axis_slabs_check.hip -- host-only check of the axis slabs of the Phase-A filter program (filter_build.h; tests/test_axis_slabs_host.py builds it
// plain and under AddressSanitizer + UBSan).  No GPU call is made.
//  1. the Cornell box's program: 1 x slab, 2 y slabs, 1 z slab in front of the aperture plane, every object once in `order`, every axis-slab
//     record in the reduced form the device's axis loops assume;
//  2. what must NOT be classed: a box rotated about y, rectangles turned within an axis plane, a normal of 1 - 2^-24, a scene without slabs;
//  3. a host restatement of Phase A's plane part in both forms -- the axis loops, and the general slab loop on the same records -- with fmaf
//     and one reciprocal fed to both: equal candidate bits on random rays and on rays with zero, subnormal, infinite and NaN components,
//     nearly parallel to the slabs, and from outside the model box.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../amber_amd/csrc/amber/rendering.h"
#include "../../amber_amd/csrc/amber/scene.h"
#include "../../amber_amd/csrc/hip/scene_prep.h"

using amber_dev::DevObject;
using amber_dev::DevPlane;
using amber_dev::DevTriFilter;
using amber_filter::FilterProgram;

static void Require(bool ok, const char* what, const char* check) {
  if (!ok) { std::printf("FAIL %s: %s\n", what, check); std::exit(1); }
}

struct Model { float center[3]; float reach, tmax; };   // DevScene's fp_center, fp_reach, fp_tmax

struct P3 { double x, y, z; };
static DevObject Triangle(P3 a, P3 b, P3 c) {
  DevObject o; std::memset(&o, 0, sizeof o);
  o.kind = AMBER_PRIM_TRIANGLE;
  const float A[3] = {float(a.x), float(a.y), float(a.z)}, B[3] = {float(b.x), float(b.y), float(b.z)}, C[3] = {float(c.x), float(c.y), float(c.z)};
  for (int k = 0; k < 3; k++) { o.a[k] = A[k]; o.e1[k] = B[k] - A[k]; o.e2[k] = C[k] - A[k]; }
  return o;
}
static void Quad(std::vector<DevObject>& objs, P3 a, P3 b, P3 c, P3 d) { objs.push_back(Triangle(a, b, c)); objs.push_back(Triangle(a, c, d)); }
// the six faces of the box centre + R [-h, h], R = rotation by `deg` about y
static void Box(std::vector<DevObject>& objs, P3 centre, P3 h, double deg) {
  const double cs = std::cos(deg * 3.14159265358979323846 / 180.0), sn = std::sin(deg * 3.14159265358979323846 / 180.0);
  auto at = [&](int sx, int sy, int sz) {
    const double x = sx * h.x, y = sy * h.y, z = sz * h.z;
    return deg == 0.0 ? P3{centre.x + x, centre.y + y, centre.z + z} : P3{centre.x + cs * x + sn * z, centre.y + y, centre.z - sn * x + cs * z};
  };
  Quad(objs, at(-1, -1, -1), at(-1, -1, 1), at(-1, 1, 1), at(-1, 1, -1)); Quad(objs, at(1, -1, -1), at(1, 1, -1), at(1, 1, 1), at(1, -1, 1));
  Quad(objs, at(-1, -1, -1), at(1, -1, -1), at(1, -1, 1), at(-1, -1, 1)); Quad(objs, at(-1, 1, -1), at(-1, 1, 1), at(1, 1, 1), at(1, 1, -1));
  Quad(objs, at(-1, -1, -1), at(-1, 1, -1), at(1, 1, -1), at(1, -1, -1)); Quad(objs, at(-1, -1, 1), at(1, -1, 1), at(1, 1, 1), at(-1, 1, 1));
}
static DevObject Sphere(P3 c, double r) {
  DevObject o; std::memset(&o, 0, sizeof o);
  o.kind = AMBER_PRIM_SPHERE; o.a[0] = float(c.x); o.a[1] = float(c.y); o.a[2] = float(c.z); o.radius = float(r);
  return o;
}
// centre, reach and largest hit distance of a scene, as PrepareScene derives them from the objects' bounds
static Model ModelOf(const std::vector<DevObject>& objs) {
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  auto grow = [&](double x, double y, double z) { const double p[3] = {x, y, z}; for (int c = 0; c < 3; c++) { lo[c] = std::min(lo[c], p[c]); hi[c] = std::max(hi[c], p[c]); } };
  for (const DevObject& o : objs) {
    if (o.kind == AMBER_PRIM_TRIANGLE) {
      grow(o.a[0], o.a[1], o.a[2]); grow(double(o.a[0]) + o.e1[0], double(o.a[1]) + o.e1[1], double(o.a[2]) + o.e1[2]); grow(double(o.a[0]) + o.e2[0], double(o.a[1]) + o.e2[1], double(o.a[2]) + o.e2[2]);
    } else { const double r = std::fabs(double(o.radius)); grow(o.a[0] - r, o.a[1] - r, o.a[2] - r); grow(o.a[0] + r, o.a[1] + r, o.a[2] + r); }
  }
  Model m{}; double reach = 0;
  for (int c = 0; c < 3; c++) { m.center[c] = float(0.5 * (lo[c] + hi[c])); reach = std::max(reach, 0.5 * (hi[c] - lo[c])); }
  m.reach = float(2.0 * reach + 1e-3); m.tmax = float(1.7320508 * 1.5 * 1.01 * double(m.reach));
  return m;
}

// ---- Phase A's plane part, restated (dev_two_phase.h: PhaseA; the spheres' filter is the same code in both forms and is left out) ----
struct PlaneState { float tp, kr, ptol, mtol; bool t_ok, degenerate, t_sure; };
static PlaneState PlaneTests(const DevPlane& pl, float nd, float no, float rc, float t_upper) {
  PlaneState s;
  s.tp = (pl.d0 - no) * rc;
  const float rho = std::fabs(rc);
  s.kr = pl.kt * rho;
  s.t_ok = (s.tp >= AMBER_KEPS - s.kr) && !(s.tp - s.kr > t_upper);
  s.degenerate = !(std::fabs(nd) >= 1e-6f);
  const bool grazing = !(std::fabs(nd) >= AMBER_GRAZING);
  s.t_sure = (s.tp - s.kr > AMBER_KEPS) && !grazing;
  s.ptol = pl.ktol * rho;
  s.mtol = grazing ? -3.402823466e+38f : -s.ptol;
  return s;
}
static bool PairTests(const PlaneState& s, float b, float a, uint32_t bit, uint32_t& cand) {   // returns plane_hit
  const float ba = b + a, g = 1.0f - ba;
  const float m1 = fminf(fminf(b, a), g), m2 = fminf(fminf(-b, 1.0f - a), ba);
  const bool keep1 = (!(m1 < s.mtol) && s.t_ok) || s.degenerate, keep2 = (!(m2 < s.mtol) && s.t_ok) || s.degenerate;
  cand |= keep1 ? bit : 0u; cand |= keep2 ? (bit << 1) : 0u;
  return fmaxf(m1, m2) >= s.ptol;
}
static float Row(const DevTriFilter& f, int row, const float P[3]) { return fmaf(f.c[0][row], P[0], fmaf(f.c[1][row], P[1], fmaf(f.c[2][row], P[2], f.c[3][row]))); }
static uint32_t PhaseAPlanes(const FilterProgram& fp, const Model& m, bool axis_loops, const float ow[3], const float d[3]) {
  const float o[3] = {ow[0] - m.center[0], ow[1] - m.center[1], ow[2] - m.center[2]};
  const float dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  float t_upper = m.tmax * (1.0f / std::sqrt(dd));
  if (!(t_upper == t_upper)) t_upper = 3.402823466e+38f;
  uint32_t cand = fp.always_mask, bit = 1u;
  size_t p = 0, rec = 0;
  float nd = 0.f, no = 0.f, rc = 0.f;
  if (axis_loops)
    for (int loop = 0; loop < 3; loop++) {
      const int c = amber_filter::AxisSlabOrder(loop);
      int u, v; amber_filter::AxisSlabInPlane(c, u, v);
      for (uint32_t k = 0; k < 2u * fp.n_axis_slabs[c]; k++, p++, rec++, bit <<= 2) {
        nd = d[c]; no = o[c]; rc = 1.0f / nd;
        const DevPlane& pl = fp.planes[p]; const DevTriFilter& f = fp.tris[rec];
        const PlaneState s = PlaneTests(pl, nd, no, rc, t_upper);
        const float Pu = fmaf(s.tp, d[u], o[u]), Pv = fmaf(s.tp, d[v], o[v]);
        const float b = fmaf(f.c[u][0], Pu, fmaf(f.c[v][0], Pv, f.c[3][0])), a = fmaf(f.c[u][1], Pu, f.c[3][1]);
        if (PairTests(s, b, a, bit, cand) && s.t_sure) t_upper = fminf(t_upper, s.tp + s.kr);
      }
    }
  auto normal = [&](const DevPlane& pl) {
    nd = fmaf(pl.n[0], d[0], fmaf(pl.n[1], d[1], pl.n[2] * d[2]));
    no = fmaf(pl.n[0], o[0], fmaf(pl.n[1], o[1], pl.n[2] * o[2]));
    rc = 1.0f / nd;
  };
  for (; p < fp.n_simple_planes; p++, rec++, bit <<= 2) {            // the general slab loop
    const DevPlane& pl = fp.planes[p];
    if ((p & 1u) == 0u) normal(pl);
    const PlaneState s = PlaneTests(pl, nd, no, rc, t_upper);
    const float P[3] = {fmaf(s.tp, d[0], o[0]), fmaf(s.tp, d[1], o[1]), fmaf(s.tp, d[2], o[2])};
    if (PairTests(s, Row(fp.tris[rec], 0, P), Row(fp.tris[rec], 1, P), bit, cand) && s.t_sure) t_upper = fminf(t_upper, s.tp + s.kr);
  }
  for (; p < fp.planes.size(); p++) {                                 // the general planes
    const DevPlane& pl = fp.planes[p];
    if (!(pl.n_tris & 0x80000000u)) normal(pl);
    const PlaneState s = PlaneTests(pl, nd, no, rc, t_upper);
    const float P[3] = {fmaf(s.tp, d[0], o[0]), fmaf(s.tp, d[1], o[1]), fmaf(s.tp, d[2], o[2])};
    bool plane_hit = false;
    for (uint32_t k = 0; k < pl.n_pairs; k++, rec++, bit <<= 2) plane_hit |= PairTests(s, Row(fp.tris[rec], 0, P), Row(fp.tris[rec], 1, P), bit, cand);
    for (uint32_t k = 0; k < (pl.n_tris & 0x7fffffffu); k++, rec++, bit <<= 1) {
      const float u = Row(fp.tris[rec], 0, P), v = Row(fp.tris[rec], 1, P), w = 1.0f - u - v;
      const float mn = fminf(fminf(u, v), w);
      cand |= ((!(mn < s.mtol) && s.t_ok) || s.degenerate) ? bit : 0u;
      plane_hit |= mn >= s.ptol;
    }
    if (plane_hit && s.t_sure) t_upper = fminf(t_upper, s.tp + s.kr);
  }
  const bool in_model = std::fabs(ow[0] - m.center[0]) <= m.reach && std::fabs(ow[1] - m.center[1]) <= m.reach && std::fabs(ow[2] - m.center[2]) <= m.reach && dd <= 4.0f;   // NaN -> false
  if (!in_model) cand = fp.order.size() >= 32 ? 0xffffffffu : ((1u << fp.order.size()) - 1u);
  return cand;
}

// the program of a scene, checked: every member once in `order`, slab counts consistent, every axis-slab record in the reduced form
static FilterProgram Build(const std::vector<DevObject>& objs, const Model& m, const char* what) {
  FilterProgram fp;
  amber_filter::BuildFilterProgram(objs, m.center, fp);
  const size_t n = std::min<size_t>(objs.size(), 32);
  std::vector<int> seen(n, 0);
  Require(fp.order.size() == n, what, "order: one slot per object");
  for (uint32_t idx : fp.order) { Require(idx < n, what, "order: index"); seen[idx]++; }
  for (int c : seen) Require(c == 1, what, "order: every object once");
  const uint32_t n_axis = fp.n_axis_slabs[0] + fp.n_axis_slabs[1] + fp.n_axis_slabs[2];
  Require(fp.n_simple_planes % 2 == 0 && 2 * n_axis <= fp.n_simple_planes && fp.n_simple_planes <= fp.planes.size(), what, "slab counts");
  const uint32_t ends = amber_filter::SlabEnds(fp);
  Require((ends >> 24) == fp.n_simple_planes && ((ends >> 16) & 0xffu) == 2 * n_axis, what, "slab_ends");
  size_t p = 0;
  for (int loop = 0; loop < 3; loop++)
    for (uint32_t k = 0, c = amber_filter::AxisSlabOrder(loop); k < 2u * fp.n_axis_slabs[c]; k++, p++) {
      const DevPlane& pl = fp.planes[p]; const DevTriFilter& f = fp.tris[p];
      int u, v; amber_filter::AxisSlabInPlane(c, u, v);
      uint32_t nbits[3]; std::memcpy(nbits, pl.n, sizeof nbits);
      Require(nbits[c] == 0x3f800000u && nbits[u] == 0u && nbits[v] == 0u, what, "axis slab: the normal is +e_c, bit for bit");
      Require(pl.n_pairs == 1 && (pl.n_tris & 0x7fffffffu) == 0, what, "axis slab: one pair record");
      Require(f.c[c][0] == 0.0f && f.c[c][1] == 0.0f && f.c[v][1] == 0.0f && f.c[u][1] != 0.0f, what, "axis slab: zero coefficients");
      Require(amber_filter::AxisSlabClass(pl, f) == c, what, "axis slab: class");
    }
  return fp;
}

struct RaySet { std::vector<float> o, d; void add(const float* oo, const float* dd) { o.insert(o.end(), oo, oo + 3); d.insert(d.end(), dd, dd + 3); } size_t size() const { return o.size() / 3; } };
static RaySet Rays(const Model& m, size_t n_random, unsigned seed) {
  RaySet r;
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> un(-1.f, 1.f);
  std::normal_distribution<float> gauss(0.f, 1.f);
  auto origin = [&](float scale, float* o) { for (int c = 0; c < 3; c++) o[c] = m.center[c] + scale * m.reach * un(rng); };
  auto direction = [&](float* d) { float l = 0; do { l = 0; for (int c = 0; c < 3; c++) { d[c] = gauss(rng); l += d[c] * d[c]; } } while (!(l > 1e-12f)); l = 1.0f / std::sqrt(l); for (int c = 0; c < 3; c++) d[c] *= l; };
  float o[3], d[3];
  for (size_t i = 0; i < n_random; i++) { origin(0.5f, o); direction(d); r.add(o, d); }               // rays of the model (the objects lie within reach / 2)
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN(), sub = 1e-40f, tiny = std::numeric_limits<float>::denorm_min();
  const float special[] = {0.0f, -0.0f, sub, -sub, tiny, -tiny, inf, -inf, nan, 1e-7f, -1e-7f, 5e-7f, -5e-7f, 9.9e-7f, 1.01e-6f, 1e-5f, -1e-5f, 5e-4f, -5e-4f, 9.9e-4f, 1.01e-3f, -1.01e-3f};
  for (int rep = 0; rep < 2000; rep++)
    for (float s : special)
      for (int c = 0; c < 3; c++) {
        origin(0.5f, o); direction(d); d[c] = s; r.add(o, d);                                             // a component of the direction: also |n.d| below 1e-6 and below AMBER_GRAZING
        if (rep % 4 == 0) { const int c2 = (c + 1) % 3; d[c2] = special[(rep / 4) % (sizeof special / sizeof special[0])]; r.add(o, d); }   // ... two of them
        if (rep % 8 == 0) { origin(0.5f, o); direction(d); o[c] = s; r.add(o, d); }                       // a component of the origin
      }
  for (int i = 0; i < 20000; i++) { origin(i % 2 ? 1.5f : 1.0f, o); direction(d); r.add(o, d); }          // origins at and beyond the edge of the model box
  for (int i = 0; i < 5000; i++) { origin(0.5f, o); direction(d); for (int c = 0; c < 3; c++) d[c] *= 2.5f; r.add(o, d); }   // |d| > 2: outside the model too
  return r;
}

// both forms on every ray: equal bits
static void CheckMasks(const FilterProgram& fp, const Model& m, size_t n_random, unsigned seed, const char* what) {
  const RaySet r = Rays(m, n_random, seed);
  size_t differ = 0, pruned = 0;
  const uint32_t tri_bits = fp.n_prog_tris >= 32 ? 0xffffffffu : ((1u << fp.n_prog_tris) - 1u);
  for (size_t i = 0; i < r.size(); i++) {
    const uint32_t a = PhaseAPlanes(fp, m, true, &r.o[3 * i], &r.d[3 * i]), g = PhaseAPlanes(fp, m, false, &r.o[3 * i], &r.d[3 * i]);
    if (a != g && differ++ < 5)
      std::printf("     ray %zu o (%a %a %a) d (%a %a %a): axis loops %08x, general loop %08x\n", i, r.o[3 * i], r.o[3 * i + 1], r.o[3 * i + 2], r.d[3 * i], r.d[3 * i + 1], r.d[3 * i + 2], a, g);
    pruned += (g & tri_bits) != tri_bits;
  }
  if (differ) { std::printf("FAIL %s: %zu of %zu rays with different candidate bits\n", what, differ, r.size()); std::exit(1); }
  Require(fp.n_prog_tris == 0 || pruned > r.size() / 2, what, "the restated filter removes candidates at all");
  std::printf("ok   masks %-34s %zu rays, slabs x %u y %u z %u of %u, %zu planes: equal bits\n", what, r.size(), fp.n_axis_slabs[0], fp.n_axis_slabs[1], fp.n_axis_slabs[2],
              fp.n_simple_planes / 2, fp.planes.size());
}

int main() {
  (void)amber_prep::ReadEnv();
  // 1. the Cornell box, as amber_hip_pt_create prepares it
  {
    const auto cornell = amber::etude::CornelBox(0.050f, 0.050f, 6).Flatten();
    const AmberSensor sensor{64, 48, 0.036f, 0.024f};
    AmberPtParams params{}; params.engine = AMBER_ENGINE_AUTO;
    const amber_prep::PreparedScene prep = amber_prep::PrepareScene(&cornell.flat, &sensor, &params, amber_prep::EnvSwitches(), 12, 52);
    Require(prep.error.empty() && prep.hit_engine == AMBER_ENGINE_TWO_PHASE, "cornell", "prepared for engine TWO_PHASE");
    Model m{};
    for (int c = 0; c < 3; c++) m.center[c] = prep.scene.fp_center[c];
    m.reach = prep.scene.fp_reach; m.tmax = prep.scene.fp_tmax;
    const FilterProgram fp = Build(prep.objects, m, "cornell");
    Require(fp.planes.size() == 9 && fp.n_simple_planes == 8, "cornell", "9 planes, 8 of them in slabs");
    Require(fp.n_axis_slabs[0] == 1 && fp.n_axis_slabs[1] == 2 && fp.n_axis_slabs[2] == 1, "cornell", "1 x slab, 2 y slabs, 1 z slab");
    Require(prep.scene.slab_ends == amber_filter::SlabEnds(fp) && (prep.scene.slab_ends >> 16) == (8u | 8u << 8), "cornell", "the scene record's slab_ends");
    Require(prep.planes.size() == fp.planes.size() && std::memcmp(prep.planes.data(), fp.planes.data(), fp.planes.size() * sizeof(DevPlane)) == 0 &&
            std::memcmp(prep.tri_filters.data(), fp.tris.data(), fp.tris.size() * sizeof(DevTriFilter)) == 0, "cornell", "the prepared records are this program");
    std::printf("ok   cornell: 1 x slab, 2 y slabs, 1 z slab, the aperture plane general\n");
    CheckMasks(fp, m, 1000000, 1, "cornell");
  }
  // 2. not axis slabs
  {
    std::vector<DevObject> objs;
    Box(objs, P3{0.1, -0.2, 0.05}, P3{0.3, 0.5, 0.2}, 30.0);
    const Model m = ModelOf(objs);
    const FilterProgram fp = Build(objs, m, "box rotated about y");
    Require(fp.n_simple_planes >= 2, "box rotated about y", "top and bottom form a slab (the other faces do where their rounded normals agree)");
    Require(fp.n_axis_slabs[0] + fp.n_axis_slabs[1] + fp.n_axis_slabs[2] == 0, "box rotated about y", "no axis slab (top and bottom have an axis normal but rotated edges)");
    bool y_normal = false;
    for (const DevPlane& pl : fp.planes) y_normal = y_normal || (std::fabs(pl.n[1]) == 1.0f && pl.n[0] == 0.0f && pl.n[2] == 0.0f);
    Require(y_normal, "box rotated about y", "top and bottom do have an exact axis normal (the case is about their rows)");
    CheckMasks(fp, m, 1000000, 2, "box rotated about y");
  }
  {
    std::vector<DevObject> objs;                                       // two squares in planes y = const, turned by 45 degrees within them
    for (double y : {-0.5, 0.5}) Quad(objs, P3{1, y, 0}, P3{0, y, 1}, P3{-1, y, 0}, P3{0, y, -1});
    const Model m = ModelOf(objs);
    const FilterProgram fp = Build(objs, m, "rectangles turned in their plane");
    Require(fp.n_simple_planes == 2 && fp.n_axis_slabs[0] + fp.n_axis_slabs[1] + fp.n_axis_slabs[2] == 0, "rectangles turned in their plane", "one slab, not an axis slab");
    CheckMasks(fp, m, 1000000, 3, "rectangles turned in their plane");
  }
  {
    std::vector<DevObject> objs;                                       // two rectangles tilted about z by 2^-11.5 rad: the normal's y rounds to 1 - 2^-24
    const double th = std::ldexp(1.0, -11) / std::sqrt(2.0), cs = std::cos(th), sn = std::sin(th);
    for (double y : {-0.5, 0.5}) Quad(objs, P3{-cs, y - sn, -1}, P3{-cs, y - sn, 1}, P3{cs, y + sn, 1}, P3{cs, y + sn, -1});
    const Model m = ModelOf(objs);
    const FilterProgram fp = Build(objs, m, "normal of 1 - 2^-24");
    uint32_t bits = 0; float ny = std::fabs(fp.planes.at(0).n[1]); std::memcpy(&bits, &ny, 4);
    Require(bits == 0x3f7fffffu, "normal of 1 - 2^-24", "the stored normal's y is 1 - 2^-24 (the case is built for that)");
    Require(fp.n_simple_planes == 2 && fp.n_axis_slabs[0] + fp.n_axis_slabs[1] + fp.n_axis_slabs[2] == 0, "normal of 1 - 2^-24", "one slab, not an axis slab");
    CheckMasks(fp, m, 1000000, 4, "normal of 1 - 2^-24");
  }
  {
    std::vector<DevObject> objs;                                       // no slab at all: lone triangles, one quad, spheres
    std::mt19937 rng(9); std::uniform_real_distribution<double> un(-1.0, 1.0);
    for (int i = 0; i < 9; i++) { const P3 a{un(rng), un(rng), un(rng)}; objs.push_back(Triangle(a, P3{a.x + 0.4 * un(rng), a.y + 0.4 * un(rng), a.z + 0.4 * un(rng)}, P3{a.x + 0.4 * un(rng), a.y + 0.4 * un(rng), a.z + 0.4 * un(rng)})); }
    Quad(objs, P3{-1, -1, -1}, P3{-1, -1, 1}, P3{1, -1, 1}, P3{1, -1, -1});
    objs.push_back(Sphere(P3{0.2, 0.1, -0.3}, 0.25)); objs.push_back(Sphere(P3{-0.4, 0.5, 0.3}, 0.1));
    const Model m = ModelOf(objs);
    const FilterProgram fp = Build(objs, m, "no slab");
    Require(fp.n_simple_planes == 0 && fp.n_axis_slabs[0] == 0 && fp.n_axis_slabs[1] == 0 && fp.n_axis_slabs[2] == 0 && amber_filter::SlabEnds(fp) == 0u, "no slab", "three zero counts");
    CheckMasks(fp, m, 1000000, 5, "no slab");
  }
  // 3. axis and other slabs together: a room of six walls and a ceiling light, with a box rotated about y and an upright box in it
  {
    std::vector<DevObject> objs;
    Box(objs, P3{0, 0, 0}, P3{1, 1, 1}, 0.0);
    Quad(objs, P3{-0.3, 0.98, -0.3}, P3{-0.3, 0.98, 0.3}, P3{0.3, 0.98, 0.3}, P3{0.3, 0.98, -0.3});
    Box(objs, P3{-0.35, -0.7, 0.2}, P3{0.25, 0.3, 0.25}, 30.0);
    objs.resize(objs.size() - 4);                                      // (without its z faces: 32 objects hold no more)
    Box(objs, P3{0.45, -0.8, -0.3}, P3{0.2, 0.2, 0.2}, 0.0);
    objs.resize(32);
    const Model m = ModelOf(objs);
    const FilterProgram fp = Build(objs, m, "room with boxes");
    const uint32_t n_axis = fp.n_axis_slabs[0] + fp.n_axis_slabs[1] + fp.n_axis_slabs[2];
    Require(fp.n_axis_slabs[0] >= 1 && fp.n_axis_slabs[1] >= 1 && fp.n_axis_slabs[2] >= 1 && fp.n_simple_planes > 2 * n_axis, "room with boxes", "axis slabs of every axis and other slabs");
    CheckMasks(fp, m, 1000000, 6, "room with boxes");
  }
  std::printf("ALL OK\n");
  return 0;
}

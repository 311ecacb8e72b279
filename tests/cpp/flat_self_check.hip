// flat_self_check.hip -- host-only check of the flat-self shortcut of the two-phase engine (filter_build.h: FlatSelfTriangle, MarkFlatSelf;
// tests/test_flat_self_host.py builds it plain and under AddressSanitizer + UBSan).  No GPU call is made.
//  (a) the classification: the Cornell box's program triangles that lie in axis planes are all marked (the count is printed) and nothing else in
//      its records changes; nothing is marked in a box rotated about y, in a tilted room, on a triangle with a 2^41 coordinate or on a non-finite
//      record; -0 edge components and A_c = -0 are marked;
//  (b) the theorem of filter_build.h: on marked triangles, for every (u, v) the acceptance tests of IntersectTriangle let through and every
//      direction bit pattern, a restatement of ResolveHit's pos and of IntersectTriangle from that pos never accepts the start triangle, and its t
//      and the self trip's t are +-0 or NaN.  A tilted control shows that the check can fail.
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

static void Require(bool ok, const char* what, const char* check) {
  if (!ok) { std::printf("FAIL %s: %s\n", what, check); std::exit(1); }
}
static uint32_t Bits(float x) { uint32_t b; std::memcpy(&b, &x, 4); return b; }
static float FromBits(uint32_t b) { float x; std::memcpy(&x, &b, 4); return x; }

struct P3 { double x, y, z; };
static DevObject Triangle(P3 a, P3 b, P3 c) {
  DevObject o; std::memset(&o, 0, sizeof o);
  o.kind = AMBER_PRIM_TRIANGLE;
  const float A[3] = {float(a.x), float(a.y), float(a.z)}, B[3] = {float(b.x), float(b.y), float(b.z)}, C[3] = {float(c.x), float(c.y), float(c.z)};
  for (int k = 0; k < 3; k++) { o.a[k] = A[k]; o.e1[k] = B[k] - A[k]; o.e2[k] = C[k] - A[k]; }
  return o;
}
static void Quad(std::vector<DevObject>& objs, P3 a, P3 b, P3 c, P3 d) { objs.push_back(Triangle(a, b, c)); objs.push_back(Triangle(a, c, d)); }
// the six faces of the box centre + R [-h, h]; R = rotation by `deg_y` about y, then by `deg_z` about z
static void Box(std::vector<DevObject>& objs, P3 centre, P3 h, double deg_y, double deg_z = 0.0) {
  const double pi = 3.14159265358979323846;
  const double cy = std::cos(deg_y * pi / 180.0), sy = std::sin(deg_y * pi / 180.0), cz = std::cos(deg_z * pi / 180.0), sz = std::sin(deg_z * pi / 180.0);
  auto at = [&](int sx, int sy_, int sz_) {
    double x = sx * h.x, y = sy_ * h.y, z = sz_ * h.z;
    if (deg_y != 0.0) { const double x1 = cy * x + sy * z, z1 = -sy * x + cy * z; x = x1; z = z1; }
    if (deg_z != 0.0) { const double x1 = cz * x - sz * y, y1 = sz * x + cz * y; x = x1; y = y1; }
    return P3{centre.x + x, centre.y + y, centre.z + z};
  };
  Quad(objs, at(-1, -1, -1), at(-1, -1, 1), at(-1, 1, 1), at(-1, 1, -1)); Quad(objs, at(1, -1, -1), at(1, 1, -1), at(1, 1, 1), at(1, -1, 1));
  Quad(objs, at(-1, -1, -1), at(1, -1, -1), at(1, -1, 1), at(-1, -1, 1)); Quad(objs, at(-1, 1, -1), at(-1, 1, 1), at(1, 1, 1), at(1, 1, -1));
  Quad(objs, at(-1, -1, -1), at(-1, 1, -1), at(1, 1, -1), at(1, -1, -1)); Quad(objs, at(-1, -1, 1), at(1, -1, 1), at(1, 1, 1), at(-1, 1, 1));
}
// the axis on which both stored edges are +-0, judged here on VALUES (the classification itself looks at bit patterns), or -1
static int FlatAxis(const DevObject& o) {
  for (int c = 0; c < 3; c++) if (o.e1[c] == 0.0f && o.e2[c] == 0.0f) return c;
  return -1;
}
static uint32_t CountMarked(const std::vector<DevObject>& objs) {
  uint32_t n = 0;
  for (const DevObject& o : objs) n += amber_filter::FlatSelfTriangle(o) ? 1u : 0u;
  return n;
}

// ---- the kernels' operations, restated (dev_math.h, dev_primitives.h, dev_closest_hit.h, dev_two_phase.h); this file is built with -ffp-contract=off ----
struct F3 { float x, y, z; };
static F3 Add(F3 a, F3 b) { return F3{a.x + b.x, a.y + b.y, a.z + b.z}; }
static F3 Sub(F3 a, F3 b) { return F3{a.x - b.x, a.y - b.y, a.z - b.z}; }
static F3 Mul(float s, F3 v) { return F3{s * v.x, s * v.y, s * v.z}; }
static float Dot(F3 u, F3 v) { return u.x * v.x + u.y * v.y + u.z * v.z; }
static F3 Cross(F3 u, F3 v) { return F3{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x}; }
static F3 Ld(const float* p) { return F3{p[0], p[1], p[2]}; }
struct Outcome { bool accepted; float t_full, t_self; };
// pos = A + u E1 + v E2 (ResolveHit), then IntersectTriangle<kTie> from o = pos against an empty best (t = FLT_MAX, idx = -1: the easiest to beat), with
// its t formed whether or not u and v pass, and the self trip's t (ClosestHitTwoPhaseView)
static Outcome CastFromOwnHit(const DevObject& ob, float hu, float hv, F3 d, F3* pos_out = nullptr) {
  const F3 A = Ld(ob.a), E1 = Ld(ob.e1), E2 = Ld(ob.e2);
  const F3 o = Add(Add(A, Mul(hu, E1)), Mul(hv, E2));
  if (pos_out) *pos_out = o;
  Outcome r{false, 0.f, 0.f};
  const F3 P = Cross(d, E2);
  const float det = Dot(P, E1);
  const F3 T = Sub(o, A);
  const float u = Dot(P, T) / det;
  const F3 Q = Cross(T, E1);
  const float v = Dot(Q, d) / det;
  const float t = Dot(Q, E2) / det;
  r.t_full = t;
  if (!(u > 1.0f || u < 0.0f) && !(v > 1.0f || v < 0.0f) && !(u + v > 1.0f))
    if (!(t <= AMBER_KEPS) && std::isfinite(t) && t < 3.402823466e+38f) r.accepted = true;
  r.t_self = Dot(Cross(Sub(o, A), E1), E2) / Dot(Cross(d, E2), E1);
  return r;
}
static bool ZeroOrNan(float t) { return t == 0.0f || t != t; }

int main() {
  (void)amber_prep::ReadEnv();
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  // (a) 1. the Cornell box, as amber_hip_pt_create prepares it
  {
    const auto cornell = amber::etude::CornelBox(0.050f, 0.050f, 6).Flatten();
    const AmberSensor sensor{64, 48, 0.036f, 0.024f};
    AmberPtParams params{}; params.engine = AMBER_ENGINE_AUTO;
    const amber_prep::PreparedScene prep = amber_prep::PrepareScene(&cornell.flat, &sensor, &params, amber_prep::EnvSwitches(), 12, 52);
    Require(prep.error.empty() && prep.hit_engine == AMBER_ENGINE_TWO_PHASE, "cornell", "prepared for engine TWO_PHASE");
    const uint32_t n_tris = prep.scene.n_prog_tris;
    uint32_t marked = 0, flat = 0;
    for (size_t k = 0; k < prep.prog_objects.size(); k++) {
      const DevObject& po = prep.prog_objects[k];
      const DevObject& so = prep.objects[po.kind >> 8];
      const bool is_marked = Bits(po.radius) == AMBER_FLAT_SELF_MARK;
      if (k < n_tris) {
        Require((po.kind & 0xffu) == AMBER_PRIM_TRIANGLE, "cornell", "a program triangle is a triangle");
        const bool is_flat = FlatAxis(so) >= 0;
        flat += is_flat; marked += is_marked;
        Require(is_marked == (is_flat && AMBER_FLAT_SELF != 0), "cornell", "marked = lies in an axis plane");
        Require(is_marked || Bits(po.radius) == 0u, "cornell", "an unmarked triangle keeps a zero word");
      } else {
        Require(Bits(po.radius) == Bits(so.radius), "cornell", "records behind the program triangles keep their radius");
      }
      DevObject a = po, b = so;                          // everything but kind's index tag and the mark is the scene's record
      a.kind &= 0xffu; a.radius = 0.f; b.radius = 0.f;
      if (k >= n_tris) { a.radius = po.radius; b.radius = so.radius; }
      Require(std::memcmp(&a, &b, sizeof a) == 0, "cornell", "the LDS image differs from the scene's records in the tag and the mark only");
    }
    for (const DevObject& o : prep.objects) Require((o.kind & 0xffu) != AMBER_PRIM_TRIANGLE || Bits(o.radius) == 0u, "cornell", "engine LIST's records are untouched");
    Require(flat >= 10 && flat == n_tris, "cornell", "every program triangle of the box lies in an axis plane");
    std::printf("ok   cornell: %u of %u program triangles lie in axis planes, %u marked (AMBER_FLAT_SELF=%d)\n", flat, n_tris, marked, int(AMBER_FLAT_SELF));
  }
  // (a) 2. what must not be marked, and what must
  {
    std::vector<DevObject> objs;
    Box(objs, P3{0.1, -0.2, 0.05}, P3{0.3, 0.5, 0.2}, 30.0);
    Require(objs.size() == 12 && CountMarked(objs) == 4, "box rotated about y", "only top and bottom (edges with an exact zero y) are marked");
    for (const DevObject& o : objs) Require(amber_filter::FlatSelfTriangle(o) == (FlatAxis(o) == 1), "box rotated about y", "marked = both edges flat in y");
    objs.clear();
    Box(objs, P3{0, 0, 0}, P3{1, 1, 1}, 20.0, 15.0);                  // a room tilted about two axes, with a tilted box in it
    Box(objs, P3{0.2, -0.3, 0.1}, P3{0.2, 0.3, 0.2}, 50.0, 15.0);
    Require(CountMarked(objs) == 0, "tilted room", "nothing is marked");
    std::vector<DevObject> prog = objs;
    amber_filter::MarkFlatSelf(prog, static_cast<uint32_t>(prog.size()));
    Require(std::memcmp(prog.data(), objs.data(), objs.size() * sizeof(DevObject)) == 0, "tilted room", "the image is left as it is");
    objs.clear();
    Box(objs, P3{0, 0, 0}, P3{1, 1, 1}, 0.0);
    Require(CountMarked(objs) == 12, "upright box", "every face is marked");
    prog = objs;
    amber_filter::MarkFlatSelf(prog, 5u);                             // only the program triangles
    for (size_t k = 0; k < prog.size(); k++) Require(Bits(prog[k].radius) == (k < 5 && AMBER_FLAT_SELF ? AMBER_FLAT_SELF_MARK : 0u), "upright box", "slots below n_prog_tris only");
    const DevObject base = Triangle(P3{0.5, 0.25, -1}, P3{1.5, 0.25, -1}, P3{0.5, 0.25, 2});   // flat in y
    Require(amber_filter::FlatSelfTriangle(base), "flat triangle", "marked");
    DevObject t = base;
    t.e1[1] = -0.0f; Require(amber_filter::FlatSelfTriangle(t), "-0 edge component", "marked");
    t.e2[1] = -0.0f; t.a[1] = -0.0f; Require(amber_filter::FlatSelfTriangle(t), "-0 edges and A_c = -0", "marked");
    t = base; t.e1[1] = std::numeric_limits<float>::denorm_min(); Require(!amber_filter::FlatSelfTriangle(t), "subnormal edge component", "not marked");
    t = base; t.a[0] = std::ldexp(1.0f, 41); Require(!amber_filter::FlatSelfTriangle(t), "2^41 coordinate", "not marked");
    t = base; t.a[1] = -std::ldexp(1.0f, 40); Require(!amber_filter::FlatSelfTriangle(t), "-2^40 coordinate", "not marked (the bound is strict)");
    t = base; t.a[1] = std::nextafter(std::ldexp(1.0f, 40), 0.0f); Require(amber_filter::FlatSelfTriangle(t), "coordinate just below 2^40", "marked");
    t = base; t.e2[2] = std::ldexp(1.0f, 41); Require(!amber_filter::FlatSelfTriangle(t), "2^41 edge", "not marked");
    for (float bad : {inf, -inf, nan})
      for (int w = 0; w < 9; w++) {
        t = base; (w < 3 ? t.a[w] : (w < 6 ? t.e1[w - 3] : t.e2[w - 6])) = bad;
        Require(!amber_filter::FlatSelfTriangle(t), "non-finite record", "not marked");
      }
    t = base; t.kind = AMBER_PRIM_SPHERE; Require(!amber_filter::FlatSelfTriangle(t), "sphere", "not marked");
    std::printf("ok   classification: rotated box, tilted room, 2^40 bound, non-finite records, -0 components\n");
  }
  // (b) the theorem
  {
    std::mt19937_64 rng(20251);
    std::uniform_real_distribution<float> un(0.f, 1.f);
    std::uniform_real_distribution<double> lg(std::log(1e-3), std::log(1e4)), lg_wide(std::log(1e-30), std::log(5.0e11));   // (twice 5e11 -- the parallel edges below -- is still under 2^40 = 1.0995e12)
    std::normal_distribution<float> gauss(0.f, 1.f);
    const float sub = 1e-40f, tiny = std::numeric_limits<float>::denorm_min();
    const float uv_special[] = {0.0f, -0.0f, 1.0f, sub, tiny, 0.5f, std::nextafter(1.0f, 0.0f), FromBits(0x00800000u), nan, -nan};
    const float d_special[] = {0.0f, -0.0f, sub, -sub, tiny, inf, -inf, nan, 2.5f, -3.0e38f, 1e-30f, 1.0f, -1.0f};
    auto coord = [&](bool wide) { const float m = float(std::exp(wide ? lg_wide(rng) : lg(rng))); return (rng() & 1u) ? m : -m; };
    auto pick = [&](const float* set, size_t n) { return set[rng() % n]; };
    const size_t kDraws = 1200000;
    for (int c = 0; c < 3; c++) {
      size_t nan_t = 0, nan_uv = 0, with_det0 = 0;
      for (size_t i = 0; i < kDraws; i++) {
        DevObject ob; std::memset(&ob, 0, sizeof ob);
        ob.kind = AMBER_PRIM_TRIANGLE;
        const bool wide = i % 8 == 7;
        for (int k = 0; k < 3; k++) { ob.a[k] = coord(wide); ob.e1[k] = coord(wide); ob.e2[k] = coord(wide); }
        ob.e1[c] = (rng() & 1u) ? 0.0f : -0.0f; ob.e2[c] = (rng() & 1u) ? 0.0f : -0.0f;
        if (i % 5 == 0) ob.a[c] = (rng() & 1u) ? 0.0f : -0.0f;
        if (i % 97 == 0) for (int k = 0; k < 3; k++) ob.e2[k] = ob.e1[k] * 2.0f;              // parallel edges: det = 0 for every direction
        if (i % 89 == 0) { const int k = (c + 1) % 3; ob.a[k] = std::nextafter(std::ldexp(1.0f, 40), 0.0f); ob.e1[k] = -ob.a[k]; ob.e2[(c + 2) % 3] = ob.a[k]; }   // at the bound
        Require(amber_filter::FlatSelfTriangle(ob), "theorem", "the drawn triangle is marked");
        // (u, v): what the acceptance tests let through -- [0, 1] with u + v <= 1, the special values, NaN
        float hu = (i % 3 == 0) ? pick(uv_special, sizeof uv_special / sizeof uv_special[0]) : un(rng);
        float hv = (i % 3 == 1) ? pick(uv_special, sizeof uv_special / sizeof uv_special[0]) : un(rng) * (hu == hu ? 1.0f - hu : 1.0f);
        if (i % 11 == 0) hu = FromBits(static_cast<uint32_t>(rng()) % 0x3f800001u);             // any bit pattern of [+0, 1]
        if (hu + hv > 1.0f) hv = 0.0f;
        Require(!(hu > 1.0f || hu < 0.0f) && !(hv > 1.0f || hv < 0.0f) && !(hu + hv > 1.0f), "theorem", "(u, v) passes the acceptance tests");
        F3 d;
        if (i % 4 == 0) d = F3{FromBits(uint32_t(rng())), FromBits(uint32_t(rng())), FromBits(uint32_t(rng()))};   // any bit pattern
        else {
          d = F3{gauss(rng), gauss(rng), gauss(rng)};
          const float l = 1.0f / std::sqrt(Dot(d, d)); d = Mul(l, d);
          if (i % 4 == 1) (&d.x)[rng() % 3] = pick(d_special, sizeof d_special / sizeof d_special[0]);
          if (i % 16 == 2) (&d.x)[c] = 0.0f;                                                       // a ray within the triangle's plane
        }
        F3 pos;
        const Outcome r = CastFromOwnHit(ob, hu, hv, d, &pos);
        if (hu == hu && hv == hv) Require(pos.x == pos.x && (&pos.x)[c] == ob.a[c], "theorem", "pos_c has the value of A_c");
        else { Require(pos.x != pos.x && pos.y != pos.y && pos.z != pos.z, "theorem", "a NaN u or v makes every component of pos NaN"); nan_uv++; }
        if (r.accepted || !ZeroOrNan(r.t_full) || !ZeroOrNan(r.t_self)) {
          std::printf("FAIL theorem axis %d draw %zu: accepted %d, t %a, self trip's t %a; A (%a %a %a) E1 (%a %a %a) E2 (%a %a %a) u %a v %a d (%a %a %a)\n", c, i, int(r.accepted),
                      r.t_full, r.t_self, ob.a[0], ob.a[1], ob.a[2], ob.e1[0], ob.e1[1], ob.e1[2], ob.e2[0], ob.e2[1], ob.e2[2], hu, hv, d.x, d.y, d.z);
          return 1;
        }
        nan_t += r.t_self != r.t_self;
        with_det0 += i % 97 == 0;
      }
      Require(nan_uv > 1000 && nan_t > nan_uv && with_det0 > 1000, "theorem", "NaN u / v, NaN t and det = 0 all occurred");
      std::printf("ok   theorem axis %d: %zu draws, the start triangle never accepted, t always +-0 or NaN (NaN in %zu, %zu of them from a NaN u or v)\n", c, kDraws, nan_t, nan_uv);
    }
    // the control: tilted triangles leave a non-zero numerator -- the check above can fail
    size_t nonzero = 0; const size_t kControl = 200000;
    for (size_t i = 0; i < kControl; i++) {
      DevObject ob; std::memset(&ob, 0, sizeof ob);
      ob.kind = AMBER_PRIM_TRIANGLE;
      for (int k = 0; k < 3; k++) { ob.a[k] = coord(false); ob.e1[k] = coord(false); ob.e2[k] = coord(false); }
      F3 d = F3{gauss(rng), gauss(rng), gauss(rng)};
      const Outcome r = CastFromOwnHit(ob, un(rng) * 0.5f, un(rng) * 0.5f, d);
      nonzero += !ZeroOrNan(r.t_self);
    }
    Require(nonzero > kControl / 2, "control", "tilted triangles mostly leave a non-zero t");
    std::printf("ok   control: %zu of %zu tilted triangles have a non-zero t at their own hit point\n", nonzero, kControl);
  }
  std::printf("ALL OK\n");
  return 0;
}

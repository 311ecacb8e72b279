// lens_sanitize.hip -- host-only driver built with AddressSanitizer + UBSan (tests/test_update_lens_abi.py): the records create derives from a
// lens and its aperture blades (scene_prep.h: DevLens with its constants, the DevBlade array) are the same bytes whether they are reached through
// create's path (PrepareScene on the scene with the new camera) or through amber_hip_pt_update_lens's (DeriveLensOfState on the state of a scene
// prepared with the OLD camera, given the new lens and blade records).  A thin lens and a pinhole, engine BVH asked for and chosen by AUTO.
// No GPU call is made.  The scenes come from the host object model through its C interface (include/amber_host.h, the product library).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/amber_host.h"
#include "../amber_amd/csrc/hip/scene_prep.h"

using amber_prep::PreparedScene;

static void Require(bool ok, const char* what, const char* check) {
  if (!ok) { std::printf("FAIL %s: %s\n", what, check); std::exit(1); }
}

struct Flat {
  std::vector<AmberFlatObject> objects;
  std::vector<AmberFlatMaterial> materials;
  AmberFlatScene flat{};
};

// about a hundred objects of all four kinds around the origin, seen through a lens at `transform`; n_blades == 0: a pinhole
static Flat MakeScene(const float transform[16], uint32_t n_blades) {
  std::vector<AmberFlatObject> objs;
  uint32_t state = 12345u;
  auto u = [&]() { state = state * 1664525u + 1013904223u; return static_cast<float>(state >> 8) / 16777216.0f * 2.0f - 1.0f; };
  for (uint32_t i = 0; i < 100; i++) {
    AmberFlatObject o{};
    o.kind = i % 4; o.material = i % 3;
    for (int c = 0; c < 3; c++) o.p[c] = 2.0f * u();
    if (o.kind == AMBER_PRIM_TRIANGLE) for (int c = 0; c < 3; c++) { o.p[3 + c] = o.p[c] + 0.3f * u(); o.p[6 + c] = o.p[c] + 0.3f * u(); }
    else if (o.kind == AMBER_PRIM_SPHERE) o.p[3] = 0.15f;
    else { o.p[3] = u(); o.p[4] = u(); o.p[5] = 1.5f; o.p[6] = 0.2f; o.p[7] = 0.4f; }
    objs.push_back(o);
  }
  const AmberFlatMaterial mats[3] = {{AMBER_MAT_LAMBERTIAN, {0.7f, 0.7f, 0.7f}, 0.f, 0.f}, {AMBER_MAT_DIFFUSE_LIGHT, {2.f, 2.f, 2.f}, 0.f, 0.f}, {AMBER_MAT_SPECULAR, {0.9f, 0.9f, 0.9f}, 0.f, 0.f}};
  amber_host_scene* hs = amber_host_scene_create(objs.data(), static_cast<uint32_t>(objs.size()), mats, 3, transform, 0.05f, 3.0f, 0.02f, n_blades, 0);
  Require(hs != nullptr, "scene", amber_host_last_error());
  Flat f;
  uint32_t no = 0, nm = 0;
  Require(amber_host_scene_flatten(hs, nullptr, &no, nullptr, &nm, nullptr) == 0, "scene", "flatten (counts)");
  f.objects.resize(no); f.materials.resize(nm);
  Require(amber_host_scene_flatten(hs, f.objects.data(), &no, f.materials.data(), &nm, &f.flat.lens) == 0, "scene", "flatten");
  amber_host_scene_destroy(hs);
  f.flat.objects = f.objects.data(); f.flat.n_objects = no; f.flat.materials = f.materials.data(); f.flat.n_materials = nm;
  return f;
}

static PreparedScene Prepare(const AmberFlatScene& s, uint32_t engine, const AmberSensor& sensor) {
  AmberPtParams params{};
  params.engine = engine;
  return amber_prep::PrepareScene(&s, &sensor, &params, amber_prep::EnvSwitches(), 12, 52);   // the kernels' AMBER_PATH_BVH_STACK, AMBER_BVH_SHADE_BATCH
}

static void Check(const char* what, uint32_t n_blades, uint32_t engine) {
  // camera A inside the geometry; camera B turned about y, raised and moved well outside A's scene bounds
  const float ta[16] = {1, 0, 0, 0.1f, 0, 1, 0, 0.2f, 0, 0, 1, 0.5f, 0, 0, 0, 1};
  const float tb[16] = {0.8f, 0, 0.6f, 7.5f, 0, 1, 0, -3.25f, -0.6f, 0, 0.8f, 11.0f, 0, 0, 0, 1};
  const AmberSensor sensor{32, 24, 0.036f, 0.027f};
  const Flat a = MakeScene(ta, n_blades), b = MakeScene(tb, n_blades);
  const AmberFlatThinLens& L = b.flat.lens;
  Require(a.flat.n_objects == b.flat.n_objects && a.flat.lens.n_blades == L.n_blades && a.flat.lens.first_blade_object == L.first_blade_object &&
          a.flat.lens.kind == L.kind, what, "the two cameras differ in the lens values and the blade geometry only");
  Require(L.kind == (n_blades ? AMBER_LENS_THIN : AMBER_LENS_PINHOLE) && L.n_blades == (n_blades ? n_blades : 1u), what, "lens kind");
  const PreparedScene pa = Prepare(a.flat, engine, sensor), pb = Prepare(b.flat, engine, sensor);
  Require(pa.error.empty() && pb.error.empty() && pa.hit_engine == AMBER_ENGINE_BVH && pb.hit_engine == AMBER_ENGINE_BVH, what, "engine BVH");
  Require(std::memcmp(&pa.lens, &pb.lens, sizeof pa.lens) != 0 && std::memcmp(pa.blades.data(), pb.blades.data(), pa.blades.size() * sizeof pa.blades[0]) != 0,
          what, "the cameras differ");
  // the update's path: the state of the handle created on A, the new lens and the new blade records
  amber_dev::DevLens lens;
  std::memset(&lens, 0xa5, sizeof lens);                                          // (stale bytes must not survive)
  std::vector<amber_dev::DevBlade> blades(3);                                     // (nor a stale size)
  float rect[4][3];
  amber_prep::DeriveLensOfState(pa, L, b.objects.data() + L.first_blade_object, lens, blades, rect);
  Require(std::memcmp(&lens, &pb.lens, sizeof lens) == 0, what, "DevLens: update path == create path, byte for byte");
  Require(blades.size() == pb.blades.size() && std::memcmp(blades.data(), pb.blades.data(), blades.size() * sizeof blades[0]) == 0, what,
          "DevBlade[]: update path == create path, byte for byte");
  for (const amber_dev::DevBlade& bl : blades) Require(bl.slot == -1, what, "a blade has no filter-program slot on engine BVH");
  bool finite = true;
  for (const auto& corner : rect) for (float v : corner) finite = finite && std::isfinite(v);
  Require(finite, what, "aperture rectangle");
  // and back: the derivation is a function of its arguments alone
  amber_prep::DeriveLensOfState(pb, a.flat.lens, a.objects.data() + L.first_blade_object, lens, blades, rect);
  Require(std::memcmp(&lens, &pa.lens, sizeof lens) == 0 && std::memcmp(blades.data(), pa.blades.data(), blades.size() * sizeof blades[0]) == 0, what, "B -> A");
  std::printf("ok   %-28s %u objects, %u blade(s): DevLens %zu bytes, DevBlade[] %zu bytes identical through create and update\n", what, a.flat.n_objects, L.n_blades,
              sizeof lens, blades.size() * sizeof blades[0]);
}

int main() {
  Check("thin lens (engine BVH)", 6, AMBER_ENGINE_BVH);
  Check("thin lens (AUTO)", 6, AMBER_ENGINE_AUTO);
  Check("thin lens, 3 blades (BVH)", 3, AMBER_ENGINE_BVH);
  Check("pinhole (engine BVH)", 0, AMBER_ENGINE_BVH);
  Check("pinhole (AUTO)", 0, AMBER_ENGINE_AUTO);
  std::printf("ALL OK\n");
  return 0;
}

// host_sanitize.hip -- host-only driver built with AddressSanitizer + UBSan (tests/test_host_sanitizers.py):
// exercises the host code that prepares device data -- object model, Flatten, the product's own scene preparation
// (scene_prep.h: engine choice, device records, filter programs and their groups, BVH builds, light slots, lens
// constants), output writers -- on degenerate and large inputs.  No GPU call is made (GPU sanitizers are not available on this pool).
#include <cstdio>
#include <random>
#include <vector>

#include <fstream>
#include <string>
#include "../amber_amd/csrc/amber/import.h"
#include "../amber_amd/csrc/amber/postprocess.h"
#include "../amber_amd/csrc/amber/rendering.h"
#include "../amber_amd/csrc/amber/scene.h"
#include "../amber_amd/csrc/hip/scene_prep.h"

using amber_dev::DevObject;
using amber_prep::PreparedScene;

static void Require(bool ok, const char* what, const char* check) {
  if (!ok) { std::printf("FAIL %s: %s\n", what, check); std::exit(1); }
}

// what amber_hip_pt_create prepares for this scene and engine (default switches), before it touches the device
static PreparedScene Prepare(const AmberFlatScene& s, uint32_t engine) {
  const AmberSensor sensor{64, 48, 0.036f, 0.024f};
  AmberPtParams params{};
  params.engine = engine;
  return amber_prep::PrepareScene(&s, &sensor, &params, amber_prep::EnvSwitches(), 12, 52);   // the kernels' AMBER_PATH_BVH_STACK, AMBER_BVH_SHADE_BATCH
}

// The prepared scene is consistent: the engine resolved as expected, every object once in the filter programs' LDS image (scene index
// in kind >> 8) and in engine BVH's leaf order, group ranges inside the merged records, every blade's and light's slot naming that
// object, finite lens constants.
static void CheckPrepared(const AmberFlatScene& s, const PreparedScene& p, uint32_t hit_engine, const char* what) {
  const uint32_t n = s.n_objects;
  Require(p.error.empty() && p.hit_engine == hit_engine, what, "engine resolution");
  Require(p.objects.size() == n && p.materials.size() == s.n_materials && p.blades.size() == s.lens.n_blades && p.lights.size() == s.n_lights, what, "record counts");
  Require(p.scene.n_objects == n && p.scene.n_lights == s.n_lights && p.scene.n_lds_objects == p.prog_objects.size(), what, "scene scalars");
  const std::vector<DevObject>& prog = p.prog_objects;
  if (p.two_phase) {
    std::vector<int> seen(n, 0);
    auto see = [&](const DevObject& o) { Require((o.kind >> 8) < n, what, "LDS image: scene index"); seen[o.kind >> 8]++; };
    if (p.groups.empty()) for (const DevObject& o : prog) see(o);
    for (size_t g = 0; g < p.groups.size(); g++) {
      const amber_dev::DevFilterGroup& gr = p.groups[g];
      Require(gr.n_objects <= 32 && gr.plane_first + gr.n_planes <= p.planes.size() && gr.tri_first <= p.tri_filters.size() &&
              gr.sphere_first + gr.n_sphere_filters <= p.sphere_filters.size(), what, "group ranges");
      for (uint32_t k = 0; k < gr.n_objects; k++) see(prog[32 * g + k]);
    }
    for (int c : seen) Require(c == 1, what, "LDS image: every object once");
    Require(p.groups.empty() == (hit_engine != amber_prep::kHitTwoPhaseN) && p.scene.n_groups == std::max<size_t>(1, p.groups.size()), what, "groups");
  }
  for (uint32_t i = 0; i < s.lens.n_blades; i++)
    Require(p.blades[i].slot < 0 || (size_t(p.blades[i].slot) < prog.size() && (prog[p.blades[i].slot].kind >> 8) == s.lens.first_blade_object + i), what, "blade slot");
  for (uint32_t i = 0; i < s.n_lights; i++)
    Require(p.lights[i].slot < 0 || (size_t(p.lights[i].slot) < prog.size() && (prog[p.lights[i].slot].kind >> 8) == s.lights[i].object), what, "light slot");
  if (hit_engine == AMBER_ENGINE_BVH || hit_engine == AMBER_ENGINE_REFERENCE_BVH) {
    Require(p.bvh_prims.size() == n && p.bvh_objects.size() == n && p.bvh_spheres.size() == n && (p.bvh_tris.empty() || p.bvh_tris.size() == 3 * n), what, "leaf-order arrays");
    std::vector<int> seen(n, 0);
    for (uint32_t k = 0; k < n; k++) {
      Require(p.bvh_prims[k] < n && std::memcmp(&p.bvh_objects[k], &p.objects[p.bvh_prims[k]], sizeof(DevObject)) == 0, what, "leaf-order records");
      seen[p.bvh_prims[k]]++;
    }
    for (int c : seen) Require(c == 1, what, "leaf order: every object once");
  }
  if (hit_engine == AMBER_ENGINE_REFERENCE_BVH) Require(p.ref_leaves.size() == p.ref_nodes.size() + 1, what, "reference tree");
  const amber_dev::DevLens& L = p.lens;
  bool finite = std::isfinite(L.size_over_area) && std::isfinite(L.inv_scene_area) && std::isfinite(L.sd2) && L.edge_tol > 0 && L.edge_tol <= 1;
  for (const auto& corner : p.aperture_rect) for (float v : corner) finite = finite && std::isfinite(v);
  Require(finite, what, "lens constants");
  std::printf("ok   prepare %-34s objects %6u: hit engine %u, %zu group(s), %zu planes, %zu lights%s\n", what, n, p.hit_engine, std::max<size_t>(1, p.groups.size()),
              p.planes.size(), p.lights.size(), hit_engine == AMBER_ENGINE_BVH ? (p.bvh_paths ? ", path kernel" : ", item kernel") : "");
}

// A flat scene that owns its arrays: one of the driver's scenes grown to n_objects by small spheres and triangles, with extra_lights more
// lights on the last triangles (in the grouped engine: the last groups)
struct GrownScene {
  std::vector<AmberFlatObject> objects;
  std::vector<AmberFlatLight> lights;
  AmberFlatScene flat{};
};
static GrownScene Grow(const AmberFlatScene& base, uint32_t n_objects, uint32_t extra_lights, unsigned seed) {
  GrownScene g;
  g.objects.assign(base.objects, base.objects + base.n_objects);
  if (base.n_lights) g.lights.assign(base.lights, base.lights + base.n_lights);
  std::mt19937 rng(seed); std::uniform_real_distribution<float> u(-1.f, 1.f);
  while (g.objects.size() < n_objects) {
    AmberFlatObject o{};
    o.material = static_cast<uint32_t>(g.objects.size() % base.n_materials);
    o.kind = g.objects.size() % 3 == 0 ? AMBER_PRIM_SPHERE : AMBER_PRIM_TRIANGLE;
    for (int c = 0; c < 3; c++) o.p[c] = u(rng);
    if (o.kind == AMBER_PRIM_SPHERE) o.p[3] = 0.02f;
    else for (int c = 0; c < 3; c++) { o.p[3 + c] = o.p[c] + 0.05f * u(rng); o.p[6 + c] = o.p[c] + 0.05f * u(rng); o.p[9 + c] = c == 2; }   // (the normal is only copied)
    g.objects.push_back(o);
  }
  for (uint32_t k = 0, i = n_objects; k < extra_lights && i-- > base.n_objects;) {
    if (g.objects[i].kind != AMBER_PRIM_TRIANGLE) continue;
    AmberFlatLight l{};
    l.object = i; l.cum_power = (g.lights.empty() ? 0.f : g.lights.back().cum_power) + 1.f; l.pdf_area = 1.f; l.irradiance[0] = l.irradiance[1] = l.irradiance[2] = 1.f;
    g.lights.push_back(l); k++;
  }
  g.flat = base;
  g.flat.objects = g.objects.data(); g.flat.n_objects = static_cast<uint32_t>(g.objects.size());
  g.flat.lights = g.lights.empty() ? nullptr : g.lights.data(); g.flat.n_lights = static_cast<uint32_t>(g.lights.size());
  return g;
}

static void CheckBvh(const std::vector<DevObject>& objs, const char* what) {
  const auto b = amber_bvh::BuildBvh(objs);
  // every object appears exactly once in the leaves, references are in range, depth within the device stack
  std::vector<int> seen(objs.size(), 0);
  size_t leaves = 0;
  std::vector<int32_t> stack{b.root_ref};
  while (!stack.empty()) {
    const int32_t r = stack.back(); stack.pop_back();
    if (r >= 0) {
      if (static_cast<size_t>(r) >= b.nodes.size()) { std::printf("FAIL %s: node ref out of range\n", what); std::exit(1); }
      stack.push_back(b.nodes[r].left); stack.push_back(b.nodes[r].right);
    } else {
      const uint32_t ref = static_cast<uint32_t>(-(r + 1)), first = ref >> 3, count = ref & 7u;
      leaves++;
      for (uint32_t k = 0; k < count; k++) {
        if (first + k >= b.prim_index.size()) { std::printf("FAIL %s: leaf range\n", what); std::exit(1); }
        seen[b.prim_index[first + k]]++;
      }
    }
  }
  for (int s : seen) if (s != 1) { std::printf("FAIL %s: object referenced %d times\n", what, s); std::exit(1); }
  if (b.depth > static_cast<uint32_t>(amber_bvh::kMaxDepth)) { std::printf("FAIL %s: depth %u\n", what, b.depth); std::exit(1); }
  std::printf("ok   bvh %-28s objects %zu nodes %zu leaves %zu depth %u\n", what, objs.size(), b.nodes.size(), leaves, b.depth);
}

// the builder of the reference's own tree (engine REFERENCE_BVH): every object in exactly one leaf, references in range, the flattened image
// as large as the tree says; degenerate inputs must neither crash nor loop (a node whose candidates all leave one side empty becomes a leaf)
static void CheckReferenceBvh(const std::vector<AmberFlatObject>& flat, const char* what) {
  const amber_refbvh::Tree t = amber_refbvh::Build(flat.data(), static_cast<uint32_t>(flat.size()));
  const amber_refbvh::FlatTree f = amber_refbvh::Flatten(t, flat.data());
  std::vector<int> seen(flat.size(), 0);
  for (const auto& lf : f.leaves)
    for (uint32_t k = lf.first; k < lf.first + (lf.count & amber_refbvh::kLeafCountMask); k++) {
      if (k >= t.order.size() || t.order[k] >= flat.size()) { std::printf("FAIL %s: reference tree leaf range\n", what); std::exit(1); }
      seen[t.order[k]]++;
    }
  for (int s : seen) if (s != 1) { std::printf("FAIL %s: reference tree references an object %d times\n", what, s); std::exit(1); }
  for (const auto& nd : f.nodes)
    for (int32_t r : {nd.left, nd.right})
      if (r >= static_cast<int32_t>(f.nodes.size()) || -(r + 1) >= static_cast<int32_t>(f.leaves.size())) { std::printf("FAIL %s: reference tree child\n", what); std::exit(1); }
  if (f.nodes.size() != t.n_inner || f.leaves.size() != t.n_leaves || t.n_leaves != t.n_inner + 1) { std::printf("FAIL %s: reference tree counts\n", what); std::exit(1); }
  std::printf("ok   reference bvh %-22s objects %zu inner %u leaves %u (largest %u) depth %u\n", what, flat.size(), t.n_inner, t.n_leaves, t.largest_leaf, t.depth);
}

int main(int argc, char** argv) {
  using namespace amber;
  const std::string out = argc > 1 ? argv[1] : ".";                              // where the writers and the import cases put their files
  (void)amber_prep::ReadEnv();
  // 1. Cornell box: flatten + the product's preparation for every engine, filter program
  const auto cornell = etude::CornelBox(0.050f, 0.050f, 6).Flatten();
  {
    const auto& fs = cornell;
    const PreparedScene prep = Prepare(fs.flat, AMBER_ENGINE_AUTO);
    CheckPrepared(fs.flat, prep, AMBER_ENGINE_TWO_PHASE, "cornell (auto)");
    CheckPrepared(fs.flat, Prepare(fs.flat, AMBER_ENGINE_LIST), AMBER_ENGINE_LIST, "cornell (list)");
    CheckPrepared(fs.flat, Prepare(fs.flat, AMBER_ENGINE_BVH), AMBER_ENGINE_BVH, "cornell (bvh)");
    CheckPrepared(fs.flat, Prepare(fs.flat, AMBER_ENGINE_REFERENCE_BVH), AMBER_ENGINE_REFERENCE_BVH, "cornell (reference bvh)");
    const std::vector<DevObject>& objs = prep.objects;
    amber_filter::FilterProgram fp;
    { const float zero_center[3] = {0, 0, 0}; amber_filter::BuildFilterProgram(objs, zero_center, fp); }
    uint32_t pairs = 0, singles = 0;
    for (const auto& pl : fp.planes) { pairs += pl.n_pairs; singles += pl.n_tris & 0x7fffffffu; }   // bit 31 of n_tris: same normal as the previous plane
    std::vector<int> slot_of(objs.size(), 0);
    for (uint32_t idx : fp.order) if (idx < objs.size()) slot_of[idx]++;
    bool each_once = true;
    for (int c : slot_of) each_once = each_once && c == 1;
    // every Cornell quad and the hexagonal aperture (three rhombi) pair up: 22 triangles in 11 parallelogram records
    if (fp.order.size() != objs.size() || !each_once || fp.planes.size() != 9 || fp.tris.size() != pairs + singles || 2 * pairs + singles != 22 ||
        pairs != 11 || fp.n_prog_tris != 22 || fp.spheres.size() != 3 || fp.always_mask != 0) {
      std::printf("FAIL filter program: planes %zu records %zu (pairs %u singles %u) spheres %zu always %x\n", fp.planes.size(), fp.tris.size(), pairs, singles,
                  fp.spheres.size(), fp.always_mask);
      return 1;
    }
    // slabs: an even number of leading planes, one pair each, the second of every two parallel to the first
    bool slabs_ok = fp.n_simple_planes % 2 == 0 && fp.n_simple_planes <= fp.planes.size();
    for (uint32_t i = 0; i < fp.n_simple_planes && slabs_ok; i++) {
      const auto& pl = fp.planes[i];
      slabs_ok = pl.n_pairs == 1 && (pl.n_tris & 0x7fffffffu) == 0 && ((i & 1u) == 0 || (pl.n_tris >> 31) == 1u);
    }
    if (!slabs_ok || fp.n_simple_planes != 8) { std::printf("FAIL filter program: slabs (%u leading planes)\n", fp.n_simple_planes); return 1; }
    std::printf("ok   filter program: 9 planes (4 slabs first), 22 triangles in 11 pair records, 3 spheres\n");
    CheckBvh(objs, "cornell");
    CheckReferenceBvh(fs.objects, "cornell");
    // AUTO's three ranges (<= 32 objects above, 33-80, 81-128), TWO_PHASE asked for up to 128 objects, lights in the last groups
    for (uint32_t n : {33u, 64u, 80u}) {
      const GrownScene g = Grow(fs.flat, n, 3, n);
      CheckPrepared(g.flat, Prepare(g.flat, AMBER_ENGINE_AUTO), amber_prep::kHitTwoPhaseN, ("cornell + small objects, auto, " + std::to_string(n)).c_str());
    }
    for (uint32_t n : {81u, 128u}) {
      const GrownScene g = Grow(fs.flat, n, 3, n);
      CheckPrepared(g.flat, Prepare(g.flat, AMBER_ENGINE_AUTO), AMBER_ENGINE_BVH, ("cornell + small objects, auto, " + std::to_string(n)).c_str());
      CheckPrepared(g.flat, Prepare(g.flat, AMBER_ENGINE_TWO_PHASE), amber_prep::kHitTwoPhaseN, ("cornell + small objects, two_phase, " + std::to_string(n)).c_str());
    }
    const GrownScene g = Grow(fs.flat, 1000, 8, 1000);
    CheckPrepared(g.flat, Prepare(g.flat, AMBER_ENGINE_REFERENCE_BVH), AMBER_ENGINE_REFERENCE_BVH, "cornell + small objects, ref bvh, 1000");
  }
  // 2. degenerate inputs: pinhole (zero-area triangle), one object, coincident centres, extreme coordinates
  {
    std::vector<std::unique_ptr<scene::Primitive>> prims; std::vector<std::unique_ptr<scene::RGBMaterial>> mats; std::vector<scene::RGBObject> objects;
    auto lens = scene::MakePinholeLens(scene::Matrix4(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 3, 0, 0, 0, 1), 0.05f);
    for (const auto& o : lens->ApertureObjects()) objects.emplace_back(*o);
    mats.emplace_back(scene::MakeLambertian(scene::RGB(0.5f)));
    prims.emplace_back(scene::MakeDisk(scene::Vector3(0, 0, 0), scene::Vector3(0, 1, 0), 1.0f));
    objects.emplace_back(prims.back().get(), mats.back().get());
    prims.emplace_back(scene::MakeCylinder(scene::Vector3(1, 0, 0), scene::Vector3(0, 1, 0), 0.2f, 1.0f));
    objects.emplace_back(prims.back().get(), mats.back().get());
    const auto sc = scene::RGBScene::Create<raytracer::List<float, scene::RGBObject>>(std::move(prims), std::move(mats), std::move(objects), std::move(lens));
    const auto fs = sc.Flatten();
    const PreparedScene prep = Prepare(fs.flat, AMBER_ENGINE_AUTO);
    CheckPrepared(fs.flat, prep, AMBER_ENGINE_TWO_PHASE, "pinhole+disk+cylinder (auto)");
    CheckPrepared(fs.flat, Prepare(fs.flat, AMBER_ENGINE_BVH), AMBER_ENGINE_BVH, "pinhole+disk+cylinder (bvh)");
    CheckPrepared(fs.flat, Prepare(fs.flat, AMBER_ENGINE_REFERENCE_BVH), AMBER_ENGINE_REFERENCE_BVH, "pinhole+disk+cylinder (ref bvh)");
    const std::vector<DevObject>& objs = prep.objects;
    amber_filter::FilterProgram fp;
    { const float zero_center[3] = {0, 0, 0}; amber_filter::BuildFilterProgram(objs, zero_center, fp); }
    if (fp.always_mask != 0x7u || !fp.planes.empty()) { std::printf("FAIL degenerate filter program always=%x\n", fp.always_mask); return 1; }
    std::printf("ok   degenerate scene: every object is an always-candidate\n");
    CheckBvh(objs, "pinhole+disk+cylinder");
    CheckReferenceBvh(fs.objects, "pinhole+disk+cylinder");
  }
  {
    std::vector<DevObject> one(1); std::memset(&one[0], 0, sizeof(DevObject)); one[0].kind = 1; one[0].radius = 1;
    CheckBvh(one, "single sphere");
    std::vector<DevObject> same(1000, one[0]);
    CheckBvh(same, "1000 coincident spheres");
    std::vector<DevObject> far(300, one[0]);
    for (size_t i = 0; i < far.size(); i++) { far[i].a[0] = (i % 2 ? 1e30f : -1e30f); far[i].a[1] = static_cast<float>(i); far[i].radius = 1e-30f; }
    CheckBvh(far, "extreme coordinates");
  }
  // 3. large random cloud: 200k spheres in the Cornell box's lens and lights, through the product's preparation (engine BVH)
  {
    std::mt19937 rng(3); std::uniform_real_distribution<float> u(-1.f, 1.f);
    GrownScene cloud = Grow(cornell.flat, 0, 0, 0);
    for (int i = 0; i < 200000; i++) { AmberFlatObject o{}; o.kind = AMBER_PRIM_SPHERE; o.p[0] = u(rng); o.p[1] = u(rng); o.p[2] = u(rng); o.p[3] = 0.004f; cloud.objects.push_back(o); }
    cloud.flat.objects = cloud.objects.data(); cloud.flat.n_objects = static_cast<uint32_t>(cloud.objects.size());
    const PreparedScene prep = Prepare(cloud.flat, AMBER_ENGINE_AUTO);
    CheckPrepared(cloud.flat, prep, AMBER_ENGINE_BVH, "cornell + 200k random spheres (auto)");
    CheckBvh(prep.objects, "200k random spheres");
    // the reference's tree of degenerate inputs: one object, a thousand coincident spheres (no plane separates them: one leaf), coordinates at the
    // edge of binary32 (surface areas overflow to inf, costs to NaN: a leaf), NaN centres (refused: std::sort on them is undefined), and 200k random spheres
    auto flat_sphere = [](float x, float y, float z, float r) { AmberFlatObject o{}; o.kind = AMBER_PRIM_SPHERE; o.p[0] = x; o.p[1] = y; o.p[2] = z; o.p[3] = r; return o; };
    CheckReferenceBvh(std::vector<AmberFlatObject>(1, flat_sphere(0, 0, 0, 1)), "single sphere");
    CheckReferenceBvh(std::vector<AmberFlatObject>(1000, flat_sphere(1, 2, 3, 0.5f)), "1000 coincident spheres");
    std::vector<AmberFlatObject> fl;
    fl.push_back(flat_sphere(-3e38f, 0, 0, 1e30f)); fl.push_back(flat_sphere(3e38f, 0, 0, 1e30f)); fl.push_back(flat_sphere(0, 0, 0, 1e-30f));
    CheckReferenceBvh(fl, "extreme coordinates");
    fl.clear();
    for (int i = 0; i < 64; i++) fl.push_back(flat_sphere(i % 3 == 0 ? std::nanf("") : float(i), float(i % 7), i % 5 == 0 ? std::nanf("") : 1.0f, 0.25f));
    if (amber_refbvh::CentresAreOrdered(fl.data(), static_cast<uint32_t>(fl.size())) || !amber_refbvh::CentresAreOrdered(fl.data() + 1, 1u)) { std::printf("FAIL NaN centres not detected\n"); return 1; }
    std::printf("ok   reference bvh: NaN centres are refused (std::sort on them is undefined)\n");
    // centres spaced geometrically along a line (120 octaves): the candidate planes are spaced evenly over the box, so a split peels off the few
    // objects of the top octaves.  The SAH stops it early here (depth 13); the guard behind it (kMaxDepth, Tree::too_deep) must stay silent
    fl.clear();
    for (int i = 0; i < 9000; i++) fl.push_back(flat_sphere(std::ldexp(1.0f, -(i % 120)) * (1.0f + 1e-3f * float(i / 120)), 0, 0, 1e-38f));
    {
      const amber_refbvh::Tree deep = amber_refbvh::Build(fl.data(), static_cast<uint32_t>(fl.size()));
      std::printf("ok   reference bvh of 9000 geometrically spaced spheres: depth %u, too_deep %d\n", deep.depth, int(deep.too_deep));
      if (deep.depth > amber_refbvh::kMaxDepth || deep.too_deep) { std::printf("FAIL depth guard\n"); return 1; }
    }
    fl.clear();
    for (int i = 0; i < 200000; i++) fl.push_back(flat_sphere(u(rng), u(rng), u(rng), 0.005f));
    CheckReferenceBvh(fl, "200k random spheres");
  }
  // 3b. round 5: filter programs of SUBSETS (the two-phase engine's groups of 32), triangle-leaf references, SAH figures
  {
    std::mt19937 rng(5); std::uniform_real_distribution<float> u(-1.f, 1.f);
    std::vector<DevObject> objs(100);
    for (size_t i = 0; i < objs.size(); i++) {
      DevObject& o = objs[i]; std::memset(&o, 0, sizeof o);
      if (i % 7 == 3) { o.kind = 1; o.a[0] = u(rng); o.a[1] = u(rng); o.a[2] = u(rng); o.radius = 0.05f; continue; }
      o.kind = 0; for (int c = 0; c < 3; c++) { o.a[c] = u(rng); o.e1[c] = 0.1f * u(rng); o.e2[c] = (i % 11 == 0) ? o.e1[c] : 0.1f * u(rng); }   // every 11th: zero area
    }
    const float center[3] = {0.1f, -0.2f, 0.3f};
    size_t slots = 0;
    for (size_t first = 0; first < objs.size(); first += 32) {
      std::vector<uint32_t> members;
      for (size_t k = first; k < std::min(objs.size(), first + 32); k++) members.push_back(static_cast<uint32_t>(objs.size() - 1 - k));   // any order, any subset
      amber_filter::FilterProgram fp;
      amber_filter::BuildFilterProgram(objs, center, fp, &members);
      std::vector<uint32_t> sorted_order = fp.order, sorted_members = members;
      std::sort(sorted_order.begin(), sorted_order.end()); std::sort(sorted_members.begin(), sorted_members.end());
      if (sorted_order != sorted_members || fp.order.size() > 32) { std::printf("FAIL subset filter program: %zu slots for %zu members\n", fp.order.size(), members.size()); return 1; }
      slots += fp.order.size();
    }
    std::printf("ok   filter programs of 4 subsets: %zu slots for %zu objects\n", slots, objs.size());
    const auto b = amber_bvh::BuildBvh(objs);
    const auto q = amber_bvh::QuantizeBvh(b.nodes, b.root_ref, [&](uint32_t slot) { return objs[b.prim_index[slot]].kind & 0xffu; });
    size_t tri_leaves = 0, sphere_leaves = 0, mixed = 0;
    for (const auto& nd : q.nodes)
      for (int32_t ref : {nd.left, nd.right}) {
        if (ref >= 0) continue;
        const uint32_t r = static_cast<uint32_t>(-(ref + 1)), first = r >> 4, count = r & 3u;
        bool tris = true, spheres = true;
        for (uint32_t k = 0; k < count; k++) { const uint32_t kind = objs[b.prim_index[first + k]].kind; tris = tris && kind == 0; spheres = spheres && kind == 1; }
        if (((r & 8u) != 0) != tris || ((r & 4u) != 0) != spheres || count == 0 || count > 3) { std::printf("FAIL leaf reference flags\n"); return 1; }
        tri_leaves += tris; sphere_leaves += spheres; mixed += !tris && !spheres;
      }
    const amber_bvh::BvhQuality bq = amber_bvh::MeasureBvh(b.nodes, b.root_ref);
    if (bq.leaves != tri_leaves + sphere_leaves + mixed || !(bq.inner_area >= 1.0) || bq.depth != b.depth) { std::printf("FAIL MeasureBvh: %u leaves, depth %u / %u\n", bq.leaves, bq.depth, b.depth); return 1; }
    std::printf("ok   leaf references: %zu triangle leaves, %zu sphere leaves, %zu mixed; SAH inner term %.2f\n", tri_leaves, sphere_leaves, mixed, bq.inner_area);
  }
  // 4. output stage writers
  {
    postprocess::HDRImage img(33, 17);
    for (unsigned y = 0; y < 17; y++) for (unsigned x = 0; x < 33; x++) img[prelude::Pixel(x, y)] = postprocess::HDR(0.001f * x, 0.002f * y, 0.5f);
    cli::ExportPNG(postprocess::Gamma()(postprocess::Filmic()(img)), out + "/amber_sanitize.png");
    cli::ExportEXR(img, out + "/amber_sanitize.exr");
    std::printf("ok   png/exr writers\n");
  }
  // 5. scene import: well-formed, malformed and random inputs must parse or throw, never read out of bounds
  {
    const std::string dir = out + "/amber_sanitize_import";
    (void)std::system(("mkdir -p '" + dir + "'").c_str());
    auto write = [&](const std::string& name, const std::string& text) { std::ofstream f(dir + "/" + name, std::ios::binary); f << text; };
    const std::string cam = "#camera 0 0 4 0 0 -1 0 1 0\n";
    const char* cases[] = {
        "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n",                                  // no camera
        "#camera 1 2 3\nv 0 0 0\n",                                                // short camera
        "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 9\n",                                  // index out of range
        "v 0 0 0\nv 1 0 0\nv 0 1 0\nf -1 -2 -7\n",                               // negative index out of range
        "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n",                                  // index 0
        "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1/ 2//3 3/x\n",                            // malformed corners
        "v 1e400 nan inf\nv 1 0 0\nv 0 1 0\nf 1 2 3\n",                          // overflowing / non-finite coordinates
        "v 0 0\n", "f\n", "f 1\n", "usemtl\nmtllib\no\ng\n", "\r\n\r\n#\n", "",
        "mtllib self.mtl\nusemtl a\nv 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nv 2 2 0\nf 1 2 3 4 5\nf -1 -2 -3\n",
    };
    write("self.mtl", "newmtl a\nKd 1 1\n");                                     // malformed colour -> error
    int parsed = 0, thrown = 0;
    for (size_t i = 0; i < sizeof cases / sizeof cases[0]; i++) {
      for (int with_cam = 0; with_cam < 2; with_cam++) {
        write("case.obj", (with_cam ? cam : std::string()) + cases[i]);
        try { auto sc = cli::ImportSceneBVH(dir + "/case.obj"); (void)sc.Flatten(); parsed++; } catch (const std::exception&) { thrown++; }
      }
    }
    write("self.mtl", "newmtl a\nKd 1 1 1\nKe 0 0 0\nKr 1 1 1\nPr 0.5\nKs 1 1 1\nNs 10\nillum 2\nnewmtl\nnewmtl b\nNs\n");
    try { (void)cli::ImportSceneBVH(dir + "/case.obj"); parsed++; } catch (const std::exception&) { thrown++; }
    std::mt19937 rng(11);
    const char alphabet[] = "vf 0123456789.-/e\n\n #camtlibuseongKdsr";
    for (int rep = 0; rep < 300; rep++) {
      std::string text = rep % 2 ? cam : std::string();
      const int len = static_cast<int>(rng() % 400);
      for (int k = 0; k < len; k++) text += alphabet[rng() % (sizeof alphabet - 1)];
      write("rand.obj", text);
      try { auto sc = cli::ImportSceneBVH(dir + "/rand.obj"); (void)sc.Flatten(); parsed++; } catch (const std::exception&) { thrown++; }
    }
    if (parsed == 0 || thrown == 0) { std::printf("FAIL import fuzz: parsed %d thrown %d\n", parsed, thrown); return 1; }
    std::printf("ok   scene import: %d inputs parsed, %d rejected with an exception\n", parsed, thrown);
  }
  std::printf("ALL OK\n");
  return 0;
}

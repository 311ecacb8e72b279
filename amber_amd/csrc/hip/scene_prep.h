// scene_prep.h -- host only: everything amber_hip_pt_create computes from its arguments before it touches the device -- the engine it
// resolves, the device records of the scene, engine BVH's and the reference's trees, the two-phase filter programs and their groups, the
// lights' slots, the lens constants -- as one plain struct of vectors and scalars.  No HIP runtime call: tests/host_sanitize.hip runs it
// under AddressSanitizer and UBSan.  The environment switches create reads are here too (ReadEnv), read once per handle.
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/amber_hip.h"
#include "bvh_build.h"
#include "filter_build.h"
#include "ref_bvh_build.h"
#include "scout_bound.h"

namespace amber_prep {

using namespace amber_dev;

constexpr uint32_t kHitTwoPhaseN = 5;                // hit_engine: the two-phase engine over groups of 32 objects (device: ENGINE_TWO_PHASE_N); not a public engine id
constexpr uint32_t kTwoPhaseAutoObjects = 80;        // AUTO picks the grouped two-phase engine up to this many objects: the Cornell box plus small quads, 1024^2 @ 128 spp
                                                     // (tools/object_count_curve.py, profiles/r05_object_count_curve.txt): 33 objects 8.5 ms against 16.5 for engine BVH, 64: 13.7 / 16.9,
                                                     // 73: 15.1 / 16.9, 89: 17.6 / 15.5 -- the curves cross near 80

// The environment switches, read once at create; results never depend on them.
struct EnvSwitches {
  uint32_t two_phase_auto = kTwoPhaseAutoObjects;   // AMBER_TWO_PHASE_MAX_OBJECTS: AUTO's largest scene for the grouped two-phase engine (measurement hook)
  int bvh_pool = -1;                                // AMBER_BVH_POOL=0/1 (lab build): overrides AMBER_PT_FLAG_BVH_POOL; -1: not set
  uint32_t bvh_shade_batch = 0;                     // AMBER_BVH_SHADE_BATCH in [1, 64]: pt_bvh_megakernel's shading batch (measurement hook); 0: the scene's own
  bool bvh_paths_off = false;                       // AMBER_BVH_PATHS=0: engine BVH never renders with the path-granular kernel
  uint32_t bvh_paths_max_depth = 0xffffffffu;       // AMBER_BVH_PATHS_MAX_DEPTH: ... nor a tree deeper than this (measurement hook)
  bool debug_bvh = false, debug_filter = false;     // AMBER_DEBUG_BVH / AMBER_DEBUG_FILTER set: the trees' / the filter program's shape on stderr
  bool pixel_mask = true;                           // AMBER_PIXEL_MASK=0: no per-pixel candidate masks of the primary rays
  uint32_t pixel_mask_block = 0;                    // AMBER_PIXEL_MASK_BLOCK=1/2/4: side of a mask's block of pixels (measurement hook); 0: not set
  double test_density_scale = 0;                    // AMBER_TEST_RECORD_DENSITY_SCALE: a test hook that mis-sizes the record buffer; 0: off
  uint32_t test_device_build_max_depth = 0;         // AMBER_TEST_DEVICE_BUILD_MAX_DEPTH: a test hook that lowers the depth the device build accepts, so that
                                                    // create's host fallback runs on an ordinary scene; 0: off (the limit is kMaxDepth)
};

inline EnvSwitches ReadEnv() {
  EnvSwitches e;
  const char* ev;
  if ((ev = std::getenv("AMBER_TWO_PHASE_MAX_OBJECTS")) && std::atoi(ev) >= 0) e.two_phase_auto = std::min<uint32_t>(AMBER_MAX_GROUP_OBJECTS, static_cast<uint32_t>(std::atoi(ev)));
#ifdef AMBER_LAB
  if ((ev = std::getenv("AMBER_BVH_POOL")) && (ev[0] == '0' || ev[0] == '1')) e.bvh_pool = ev[0] == '1';
#endif
  if ((ev = std::getenv("AMBER_BVH_SHADE_BATCH")) && std::atoi(ev) >= 1 && std::atoi(ev) <= 64) e.bvh_shade_batch = static_cast<uint32_t>(std::atoi(ev));
  e.bvh_paths_off = (ev = std::getenv("AMBER_BVH_PATHS")) && ev[0] == '0';
  if ((ev = std::getenv("AMBER_BVH_PATHS_MAX_DEPTH"))) e.bvh_paths_max_depth = static_cast<uint32_t>(std::atoi(ev));
  e.debug_bvh = std::getenv("AMBER_DEBUG_BVH") != nullptr;
  e.debug_filter = std::getenv("AMBER_DEBUG_FILTER") != nullptr;
  e.pixel_mask = !((ev = std::getenv("AMBER_PIXEL_MASK")) && ev[0] == '0');
  if ((ev = std::getenv("AMBER_PIXEL_MASK_BLOCK")) && (ev[0] == '1' || ev[0] == '2' || ev[0] == '4') && ev[1] == 0) e.pixel_mask_block = static_cast<uint32_t>(ev[0] - '0');
  if ((ev = std::getenv("AMBER_TEST_RECORD_DENSITY_SCALE"))) e.test_density_scale = std::atof(ev);
  if ((ev = std::getenv("AMBER_TEST_DEVICE_BUILD_MAX_DEPTH")) && std::atoi(ev) > 0) e.test_device_build_max_depth = static_cast<uint32_t>(std::atoi(ev));
  return e;
}

// What the handle keeps of the preparation (amber_hip_pt derives from it)
struct SceneState {
  uint32_t engine = AMBER_ENGINE_LIST;       // as requested / resolved: LIST, TWO_PHASE, BVH, WAVEFRONT or REFERENCE_BVH
  uint32_t hit_engine = AMBER_ENGINE_LIST;   // closest-hit engine the kernels are instantiated with
  bool two_phase = false;
  bool bvh_pool = false;                     // engine BVH renders with pt_bvh_pool_kernel (AMBER_PT_FLAG_BVH_POOL / AMBER_BVH_POOL=1) instead of pt_bvh_megakernel
  bool bvh_paths = false;                    // engine BVH on a shallow tree (depth <= AMBER_PATH_BVH_STACK): pt_megakernel<ENGINE_BVH>, the path-granular scheduler
  uint32_t bvh_shade_batch = 0;              // pt_bvh_megakernel's shading batch for this scene
  DevScene scene{};                          // every scalar field; the upload adds the pointers and ref_stack_stride
  DevLens lens{};                            // host copy of *scene.lens (pixel_mask_kernel's arguments derive from it)
  float aperture_rect[4][3] = {};            // world corners of the blades' bounding rectangle in the lens plane (pixel_mask_kernel)
  std::vector<uint32_t> prog_order;          // two-phase engine: scene index of the object in filter-program slot k (the bit positions of the masks)
  std::vector<DevPlane> host_planes;         // ... and its plane records (pixel_mask_kernel's wave-uniform tests are made on the host)
  AmberBuildInfo build{};                    // engine BVH's tree: who built it, its size, what the tree stage cost (amber_hip_pt_build_info)
};

// Engine BVH's scheduler and shading batch, from the depth of its tree -- whoever built it.
// (n_objects, n_triangles, flags: what the choice needs of the scene and of AmberPtParams.reserved -- a handle keeps them, so that a tree rebuilt
//  by amber_hip_pt_update_objects chooses again without the host's object records)
inline void ChooseBvhScheduler(SceneState& st, size_t n_objects, size_t n_triangles, uint32_t flags, const EnvSwitches& env,
                               size_t n_nodes, uint32_t depth, uint32_t path_bvh_stack, uint32_t shade_batch) {
  st.bvh_paths = !st.bvh_pool && !(flags & AMBER_PT_FLAG_BVH_ITEMS) && st.engine != AMBER_ENGINE_WAVEFRONT && depth <= path_bvh_stack;
  // The shading batch of pt_bvh_megakernel.  While a wave collects finished lanes they idle through the rounds of the others, and a round
  // over triangle leaves costs about twice a round over sphere leaves (45 against 20 vector instructions per leaf object before any
  // root / quotient), so idle lanes are dearer in a mesh: tools/shade_batch_sweep.py (profiles/r05_shade_batch_sweep.txt) -- 1M spheres
  // best at 52 (49.7 ms at 64 spp; 40: 52.3), 1M-triangle terrain at 32 (62.1; 40: 63.8; 52: 68.5), 82k-triangle room at 36-44 (32.8; 52: 33.9).
  st.bvh_shade_batch = 2u * n_triangles > n_objects ? 40u : shade_batch;   // a mesh: 40; mostly spheres (disks, cylinders): 52
  if (env.bvh_shade_batch) st.bvh_shade_batch = env.bvh_shade_batch;
  if (env.bvh_paths_off || env.bvh_paths_max_depth < depth) st.bvh_paths = false;
  if (env.debug_bvh) std::fprintf(stderr, "amber_hip: BVH of %zu objects: %zu nodes, depth %u; scheduler %s, shading batch %u\n", n_objects, n_nodes, depth,
                                  st.bvh_pool ? "pt_bvh_pool_kernel" : (st.bvh_paths ? "pt_megakernel<ENGINE_BVH>" : "pt_bvh_megakernel"), st.bvh_shade_batch);
}
inline size_t CountTriangles(const std::vector<DevObject>& objs) {   // (every scene has a few: the aperture blades)
  size_t n_triangles = 0;
  for (const DevObject& ob : objs) n_triangles += (ob.kind & 0xffu) == AMBER_PRIM_TRIANGLE ? 1u : 0u;
  return n_triangles;
}
inline void ChooseBvhScheduler(SceneState& st, const std::vector<DevObject>& objs, const AmberPtParams* params, const EnvSwitches& env,
                               size_t n_nodes, uint32_t depth, uint32_t path_bvh_stack, uint32_t shade_batch) {
  ChooseBvhScheduler(st, objs.size(), CountTriangles(objs), params->reserved, env, n_nodes, depth, path_bvh_stack, shade_batch);
}

// The host builder (bvh_build.h) and what follows from its tree's depth.
inline amber_bvh::FlatBvh BuildHostTree(SceneState& st, const std::vector<DevObject>& objs, const AmberPtParams* params, const EnvSwitches& env,
                                        uint32_t path_bvh_stack, uint32_t shade_batch) {
  const auto t0 = std::chrono::steady_clock::now();
  amber_bvh::FlatBvh bvh = amber_bvh::BuildBvh(objs);
  st.build.tree_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (env.debug_bvh) {
    const amber_bvh::BvhQuality q = amber_bvh::MeasureBvh(bvh.nodes, bvh.root_ref);
    std::fprintf(stderr, "amber_hip: BVH %s: SAH inner-node term %.3f, leaf term %.3f (x objects %.3f), leaf volume / scene volume %.3f; %u inner nodes, %u leaves, %u levels\n",
                 "as built", q.inner_area, q.leaf_area, q.leaf_object_area, q.leaf_volume, q.inner, q.leaves, q.depth);
  }
  ChooseBvhScheduler(st, objs, params, env, bvh.nodes.size(), bvh.depth, path_bvh_stack, shade_batch);
  st.build.where = st.build.fallback_reason ? AMBER_BUILD_HOST_FALLBACK : AMBER_BUILD_HOST;
  st.build.n_nodes = static_cast<uint32_t>(bvh.nodes.size()); st.build.n_leaves = st.build.n_nodes + 1u; st.build.depth = bvh.depth;
  return bvh;
}

// Per-ray box margin of engine BVH (BvhBegin) from the bounds of all widened object boxes: centre and half diagonal of the scene bounds, 1 / smallest sphere radius
inline void SetBvhRayMargin(DevScene& sc, const float bounds_min[3], const float bounds_max[3], bool has_spheres, float min_sphere_radius) {
  double d2 = 0;
  for (int c = 0; c < 3; c++) {
    sc.bvh_center[c] = 0.5f * (bounds_min[c] + bounds_max[c]);
    const double e = double(bounds_max[c]) - bounds_min[c];
    d2 += e * e;
  }
  sc.bvh_half_diag = static_cast<float>(0.5 * std::sqrt(d2) * 1.0001);
  sc.bvh_inv_rmin = !has_spheres ? 0.0f : (min_sphere_radius > 0 ? static_cast<float>(std::min(3.0e38, 1.0001 / min_sphere_radius)) : 3.0e38f);
}


// Everything create derives from the lens and its aperture blades alone (the sensor and the two-phase model box given): the DevLens record with
// its constants, the DevBlade array and the aperture's bounding rectangle.  amber_hip_pt_create (PrepareScene) and amber_hip_pt_update_lens
// (DeriveLensOfState) both come here, so the two cannot drift.  blade_records: L.n_blades records, the scene objects [L.first_blade_object, ...).
// A blade's filter-program slot is the two-phase engines' (PrepareScene assigns it); it is -1 here and stays -1 on engine BVH.
// lens and aperture_rect are written in place (the record is cleared first, padding included).
inline void DeriveLens(const AmberFlatThinLens& L, const AmberFlatObject* blade_records, const AmberSensor& sensor, const float fp_center[3], float fp_reach,
                       DevLens& lens, std::vector<DevBlade>& blades, float aperture_rect[4][3]) {
  blades.resize(L.n_blades);
  for (uint32_t i = 0; i < L.n_blades; i++) {
    const AmberFlatObject& f = blade_records[i];
    for (int c = 0; c < 3; c++) { blades[i].v0[c] = f.p[c]; blades[i].v1[c] = f.p[3 + c]; blades[i].v2[c] = f.p[6 + c]; blades[i].n[c] = f.p[9 + c]; }
    blades[i].slot = -1; blades[i].pad[0] = blades[i].pad[1] = blades[i].pad[2] = 0;
  }
  {
    // bounding rectangle of the aperture in the lens plane (lens-local x, y; the blades lie in z = 0), inflated, as four world points
    double lo[2] = {1e300, 1e300}, hi[2] = {-1e300, -1e300};
    for (const DevBlade& bl : blades)
      for (const float* v : {bl.v0, bl.v1, bl.v2}) {
        const double r[3] = {double(v[0]) - L.origin[0], double(v[1]) - L.origin[1], double(v[2]) - L.origin[2]};
        for (int c = 0; c < 2; c++) {
          const double x = L.local_[3 * c] * r[0] + L.local_[3 * c + 1] * r[1] + L.local_[3 * c + 2] * r[2];
          lo[c] = std::min(lo[c], x); hi[c] = std::max(hi[c], x);
        }
      }
    double world_mag = 0;
    for (int c = 0; c < 3; c++) world_mag = std::max({world_mag, std::fabs(double(fp_center[c])) + fp_reach, std::fabs(double(L.origin[c]))});
    for (int c = 0; c < 2; c++) { const double m = 1e-3 * (hi[c] - lo[c]) + 1e-6 + 1e-5 * fp_reach + 32.0 * 5.9604644775390625e-08 * world_mag; lo[c] -= m; hi[c] += m; }
    for (int i = 0; i < 4; i++) {
      const double x = (i & 1) ? hi[0] : lo[0], y = (i & 2) ? hi[1] : lo[1];
      for (int c = 0; c < 3; c++) aperture_rect[i][c] = static_cast<float>(L.origin[c] + (L.kind == AMBER_LENS_PINHOLE ? 0.0 : L.global_[3 * c] * x + L.global_[3 * c + 1] * y));
    }
  }
  std::memset(&lens, 0, sizeof lens);
  std::memcpy(lens.origin, L.origin, sizeof L.origin);
  std::memcpy(lens.global_, L.global_, sizeof L.global_);
  std::memcpy(lens.local_, L.local_, sizeof L.local_);
  lens.focus_distance = L.focus_distance; lens.sensor_distance = L.sensor_distance; lens.p_area = L.p_area;
  { volatile float q = -L.focus_distance / L.sensor_distance; lens.neg_fd_over_sd = q; }
  {
    // sensor.Size() / sensor.SceneArea(): uint -> float, float*float, float/float (lens_thin.cc:145, sensor.cc:40-50)
    volatile float size_f = static_cast<float>(static_cast<uint64_t>(sensor.width) * sensor.height);
    volatile float area = sensor.scene_width * sensor.scene_height;
    volatile float r = size_f / area;
    lens.size_over_area = r;
  }
  lens.sd2 = static_cast<double>(L.sensor_distance) * static_cast<double>(L.sensor_distance);
  lens.n_blades = L.n_blades; lens.n_blades_f = static_cast<float>(L.n_blades);
  lens.kind = L.kind;
  { volatile float area = sensor.scene_width * sensor.scene_height; volatile float inv = 1.0f / area; lens.inv_scene_area = inv; }
  { volatile float q = -L.sensor_distance / L.focus_distance; lens.neg_sd_over_fd = q; }
  {
    // a ray that starts on blade b is seen by another blade's exact test only if its origin lies within the rounding of WORLD
    // coordinates of that blade: a few ulp of the lens position, in units of the blade's size
    double world_mag = 0, min_edge = 1e300;
    for (int c = 0; c < 3; c++) world_mag = std::max(world_mag, std::fabs(double(L.origin[c])));
    for (const DevBlade& bl : blades) {
      const float* v[3] = {bl.v0, bl.v1, bl.v2};
      for (int k = 0; k < 3; k++) {
        double e2 = 0;
        for (int c = 0; c < 3; c++) { const double e = double(v[k][c]) - v[(k + 1) % 3][c]; e2 += e * e; world_mag = std::max(world_mag, std::fabs(double(v[k][c]))); }
        min_edge = std::min(min_edge, std::sqrt(e2));
      }
    }
    const double tol = min_edge > 0 ? std::max(1e-3, 64.0 * 5.9604644775390625e-08 * world_mag / min_edge) : 1.0;
    lens.edge_tol = static_cast<float>(std::min(1.0, tol));
  }
}

// Does this handle scout (pt_megakernel's AMBER_KERNEL_SCOUT instantiation + replay_records_kernel) -- and from which bound of the eye weight?  Only the
// 32-object two-phase engine has the instantiation; AMBER_PT_FLAG_NO_SCOUT asks for the full kernel; and the host must be able to bound the eye weight of this
// lens (scout_bound.h: a thin lens or a pinhole with finite constants in range).  A non-finite material constant sends the handle to the full kernel as well:
// the per-lane rule would flag those paths one by one, and a scene like that is no place to save arithmetic.  Decided once, at create: the handles that take
// amber_hip_pt_update_lens and amber_hip_pt_update_objects are engine BVH's, which never scout.
inline bool DecideScout(uint32_t engine, uint32_t hit_engine, uint32_t flags, const DevLens& lens, const std::vector<DevBlade>& blades, const std::vector<DevMaterial>& materials,
                        float sensor_w, float sensor_h, uint32_t* bound0) {
  *bound0 = 0;
  if (engine == AMBER_ENGINE_WAVEFRONT || hit_engine != AMBER_ENGINE_TWO_PHASE || (flags & AMBER_PT_FLAG_NO_SCOUT)) return false;   // (the lab's WAVEFRONT only borrows the hit engine)
  for (const DevMaterial& m : materials)
    for (float x : {m.rho[0], m.rho[1], m.rho[2], m.param, m.r0, m.aux0, m.aux1}) if (!std::isfinite(x)) return false;
  std::vector<float> vertices;
  for (const DevBlade& bl : blades) for (const float* v : {bl.v0, bl.v1, bl.v2}) vertices.insert(vertices.end(), v, v + 3);
  amber_scout::LensFacts f{};
  f.kind = lens.kind; f.local_ = lens.local_; f.global_ = lens.global_; f.origin = lens.origin;
  f.sensor_distance = lens.sensor_distance; f.focus_distance = lens.focus_distance; f.p_area = lens.p_area; f.size_over_area = lens.size_over_area;
  f.inv_scene_area = lens.inv_scene_area; f.sensor_w = sensor_w; f.sensor_h = sensor_h;
  f.blade_vertices = vertices.data(); f.n_vertices = static_cast<uint32_t>(vertices.size() / 3u);
  return amber_scout::EyeWeightBound(f, bound0);
}

// The same records for a new lens on a resident scene (amber_hip_pt_update_lens): the sensor is the handle's, and so is the two-phase model box --
// engine BVH, the only engine whose handles take a lens update, reads neither the box nor the rectangle whose margin derives from it.
inline void DeriveLensOfState(const SceneState& st, const AmberFlatThinLens& L, const AmberFlatObject* blade_records,
                              DevLens& lens, std::vector<DevBlade>& blades, float aperture_rect[4][3]) {
  const AmberSensor sensor{st.scene.sensor.w, st.scene.sensor.h, st.scene.sensor.sw, st.scene.sensor.sh};
  DeriveLens(L, blade_records, sensor, st.scene.fp_center, st.scene.fp_reach, lens, blades, aperture_rect);
}

struct PreparedScene : SceneState {
  std::string error;                         // not empty: create refuses the scene (AMBER_EINVAL) with this message
  bool bvh_pending = false;                  // AMBER_PT_FLAG_DEVICE_BUILD on engine BVH: no tree yet -- create builds it on the device (bvh_device_build.inc) or calls HostBvh
  uint32_t ref_depth = 0;                    // levels of the reference's tree (engine REFERENCE_BVH: its traversal stack)
  // the device arrays
  std::vector<DevObject> objects;
  std::vector<DevMaterial> materials;
  std::vector<DevBlade> blades;
  std::vector<DevPlane> planes;              // the filter programs: every group's records behind each other
  std::vector<DevTriFilter> tri_filters;
  std::vector<DevSphereFilter> sphere_filters;
  std::vector<DevObject> prog_objects;       // the LDS image: objects in program order, 32 slots per group in the grouped engine
  std::vector<DevFilterGroup> groups;        // engine TWO_PHASE_N only: one record per group of 32 objects
  std::vector<DevLight> lights;
  std::vector<DevBvhNodeQ> bvh_nodes;        // engine BVH: quantised nodes, leaf-order permutation, object records and compact sphere / triangle records in leaf order
  std::vector<DevBvhNodeQ4> bvh_nodes4;      // AMBER_BVH_WIDE builds only
  std::vector<uint32_t> bvh_prims;
  std::vector<DevObject> bvh_objects;
  std::vector<float4> bvh_spheres, bvh_tris;
  std::vector<DevRefNode> ref_nodes;         // engine REFERENCE_BVH: the reference's own tree
  std::vector<DevRefLeaf> ref_leaves;
};

// st and p are the same object while PrepareScene runs; in create's fallback (HostBvhFallback) the state has been moved into the handle and
// p still holds the arrays to upload, so the scalars go to st and the vectors to p.
// Engine BVH's device arrays from a host-built tree: quantised nodes, leaf-order permutation, object records and compact sphere / triangle
// records in leaf order, the grid and the per-ray margin.  (Engine REFERENCE_BVH: only the object arrays, in the order bvh.prim_index gives.)
inline void FillBvhArrays(SceneState& st, PreparedScene& p, const std::vector<DevObject>& objs, amber_bvh::FlatBvh& bvh) {
  const auto t0 = std::chrono::steady_clock::now();
  amber_bvh::QuantizedBvh qbvh = amber_bvh::QuantizeBvh(bvh.nodes, bvh.root_ref, [&](uint32_t slot) { return objs[bvh.prim_index[slot]].kind & 0xffu; });
#if AMBER_BVH_WIDE
  {
    amber_bvh::QuantizedBvh4 q4 = amber_bvh::CollapseBvh4(bvh.nodes, bvh.root_ref, qbvh, [&](uint32_t slot) { return objs[bvh.prim_index[slot]].kind & 0xffu; });
    p.bvh_nodes4 = std::move(q4.nodes);
    qbvh.root_ref = q4.root_ref;
  }
#endif
  p.bvh_nodes = std::move(qbvh.nodes);
  {
    std::vector<DevObject>& leaf_order = p.bvh_objects;
    std::vector<float4>& leaf_spheres = p.bvh_spheres;
    leaf_order.resize(bvh.prim_index.size());
    leaf_spheres.resize(bvh.prim_index.size());
    for (size_t k = 0; k < leaf_order.size(); k++) {
      const DevObject& ob = objs[bvh.prim_index[k]];
      leaf_order[k] = ob;
      leaf_spheres[k] = (ob.kind & 0xffu) == AMBER_PRIM_SPHERE ? make_float4(ob.a[0], ob.a[1], ob.a[2], ob.radius) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // compact triangle records of the leaves (IntersectTriangleLeaf): three float4 per leaf-order slot, only when the scene has triangles
    bool any_tri = false;
    for (const DevObject& ob : leaf_order) any_tri = any_tri || (ob.kind & 0xffu) == AMBER_PRIM_TRIANGLE;
    std::vector<float4>& leaf_tris = p.bvh_tris;
    leaf_tris.resize(any_tri ? 3 * leaf_order.size() : 0);
    for (size_t k = 0; any_tri && k < leaf_order.size(); k++) {
      const DevObject& ob = leaf_order[k];
      if ((ob.kind & 0xffu) != AMBER_PRIM_TRIANGLE) { leaf_tris[3 * k] = leaf_tris[3 * k + 1] = leaf_tris[3 * k + 2] = make_float4(0.f, 0.f, 0.f, 0.f); continue; }
      float idx; const uint32_t scene_index = bvh.prim_index[k]; std::memcpy(&idx, &scene_index, 4);
      leaf_tris[3 * k] = make_float4(ob.a[0], ob.a[1], ob.a[2], ob.e1[0]);
      leaf_tris[3 * k + 1] = make_float4(ob.e1[1], ob.e1[2], ob.e2[0], ob.e2[1]);
      leaf_tris[3 * k + 2] = make_float4(ob.e2[2], idx, 0.f, 0.f);
    }
  }
  p.bvh_prims = std::move(bvh.prim_index);
  DevScene& sc = st.scene;
  sc.bvh_root = qbvh.root_ref;
  for (int c = 0; c < 3; c++) { sc.bvh_gmin[c] = qbvh.gmin[c]; sc.bvh_step[c] = qbvh.step[c]; sc.bvh_reach[c] = qbvh.reach[c]; }
  SetBvhRayMargin(sc, bvh.bounds_min, bvh.bounds_max, bvh.has_spheres, bvh.min_sphere_radius);
  if (st.hit_engine == AMBER_ENGINE_BVH) st.build.tree_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// A scene prepared with its tree pending (AMBER_PT_FLAG_DEVICE_BUILD) whose tree the device did not build: the host builder after all.
// st: where the scene's state lives by now (create has moved it into the handle).
inline void HostBvhFallback(SceneState& st, PreparedScene& p, uint32_t reason, const AmberPtParams* params, const EnvSwitches& env, uint32_t path_bvh_stack, uint32_t shade_batch) {
  st.build.fallback_reason = reason;
  amber_bvh::FlatBvh bvh = BuildHostTree(st, p.objects, params, env, path_bvh_stack, shade_batch);
  FillBvhArrays(st, p, p.objects, bvh);
  p.bvh_pending = false;
}

// The scene, sensor and parameters are those amber_hip_pt_create has validated; path_bvh_stack and shade_batch are the kernels'
// AMBER_PATH_BVH_STACK and AMBER_BVH_SHADE_BATCH.
inline PreparedScene PrepareScene(const AmberFlatScene* s, const AmberSensor* sensor, const AmberPtParams* params, const EnvSwitches& env,
                                  uint32_t path_bvh_stack, uint32_t shade_batch) {
  PreparedScene p;
  p.bvh_shade_batch = shade_batch;
  // ---- flatten -> device layout
  std::vector<DevObject>& objs = p.objects;
  objs.resize(s->n_objects);
  for (uint32_t i = 0; i < s->n_objects; i++) {
    const AmberFlatObject& f = s->objects[i];
    DevObject& o = objs[i];
    std::memset(&o, 0, sizeof o);
    o.kind = f.kind; o.material = f.material;
    o.a[0] = f.p[0]; o.a[1] = f.p[1]; o.a[2] = f.p[2];
    if (f.kind == AMBER_PRIM_TRIANGLE) {
      // E1 = v1 - v0, E2 = v2 - v0 (primitive_triangle.cc:100-101): same binary32 subtraction the
      // reference performs per intersection, hoisted to scene upload.
      for (int c = 0; c < 3; c++) {
        volatile float e1 = f.p[3 + c] - f.p[c];
        volatile float e2 = f.p[6 + c] - f.p[c];
        o.e1[c] = e1; o.e2[c] = e2; o.n[c] = f.p[9 + c];
      }
    } else if (f.kind == AMBER_PRIM_SPHERE) {
      o.radius = f.p[3];
    } else {
      o.e1[0] = f.p[3]; o.e1[1] = f.p[4]; o.e1[2] = f.p[5]; o.radius = f.p[6]; o.height = f.p[7];
    }
  }
  p.materials.resize(s->n_materials);
  for (uint32_t i = 0; i < s->n_materials; i++) {
    const AmberFlatMaterial& f = s->materials[i];
    DevMaterial& m = p.materials[i];
    std::memset(&m, 0, sizeof m);
    m.kind = f.kind; m.rho[0] = f.rho[0]; m.rho[1] = f.rho[1]; m.rho[2] = f.rho[2]; m.param = f.param; m.r0 = f.r0;
    // constants the reference recomputes for every sample (material_phong.cc:92-105, material_refraction.cc:181-183): the same
    // binary32 operations, once (volatile: no wider intermediate, no reassociation)
    volatile float e1 = f.param + 1.0f, e2 = f.param + 2.0f;
    if (f.kind == AMBER_MAT_PHONG) { volatile float a = 1.0f / e1, b = e2 / e1; m.aux0 = a; m.aux1 = b; }
    else if (f.kind == AMBER_MAT_REFRACTION) { volatile float a = 1.0f / f.param; m.aux0 = a; }
  }
  const AmberFlatThinLens& L = s->lens;
  std::vector<DevBlade>& blades = p.blades;

  // AUTO: <= 32 objects the two-phase engine; up to env.two_phase_auto its grouped form (one Phase-A program per 32 objects: cheaper than a per-lane
  // tree traversal while the groups are few -- tools/object_count_curve.py); beyond that engine BVH.  Asked for explicitly, two-phase takes up to 128 objects.
  const uint32_t auto_hit = s->n_objects <= AMBER_MAX_LDS_OBJECTS ? AMBER_ENGINE_TWO_PHASE : (s->n_objects <= env.two_phase_auto ? kHitTwoPhaseN : AMBER_ENGINE_BVH);
  p.engine = params->engine != AMBER_ENGINE_AUTO ? params->engine : (auto_hit == kHitTwoPhaseN ? static_cast<uint32_t>(AMBER_ENGINE_TWO_PHASE) : auto_hit);
  p.hit_engine = p.engine == AMBER_ENGINE_WAVEFRONT ? (s->n_objects <= AMBER_MAX_LDS_OBJECTS ? AMBER_ENGINE_TWO_PHASE : AMBER_ENGINE_BVH) : p.engine;
  if (p.hit_engine == AMBER_ENGINE_TWO_PHASE && s->n_objects > AMBER_MAX_LDS_OBJECTS) p.hit_engine = kHitTwoPhaseN;
  p.two_phase = p.hit_engine == AMBER_ENGINE_TWO_PHASE || p.hit_engine == kHitTwoPhaseN;
  // engine BVH has two schedulers with identical results: the default is the faster one on the 1M-sphere
  // scene (pt_bvh_megakernel, 74 ms at 64 spp against 79); the environment overrides the flag either way (A/B tools)
#ifdef AMBER_LAB
  p.bvh_pool = env.bvh_pool >= 0 ? env.bvh_pool == 1 : (params->reserved & AMBER_PT_FLAG_BVH_POOL) != 0u;
#endif
  amber_bvh::FlatBvh bvh;
  if (p.hit_engine == AMBER_ENGINE_BVH) {
    const bool device_build = (params->reserved & AMBER_PT_FLAG_DEVICE_BUILD) != 0u;
#if AMBER_BVH_WIDE
    if (device_build) p.build.fallback_reason = AMBER_BUILD_REASON_WIDE;   // the device builder writes 2-wide nodes only
    bvh = BuildHostTree(p, objs, params, env, path_bvh_stack, shade_batch);
#else
    if (device_build) p.bvh_pending = true;
    else bvh = BuildHostTree(p, objs, params, env, path_bvh_stack, shade_batch);
#endif
  }
  amber_refbvh::FlatTree ref_tree;
  if (p.hit_engine == AMBER_ENGINE_REFERENCE_BVH) {
    const amber_refbvh::Tree tree = amber_refbvh::Build(s->objects, s->n_objects);
    if (tree.too_deep) { p.error = "AMBER_ENGINE_REFERENCE_BVH: the reference's recursive build goes deeper than " + std::to_string(amber_refbvh::kMaxDepth) + " levels on this scene"; return p; }
    ref_tree = amber_refbvh::Flatten(tree, s->objects);
    p.ref_depth = tree.depth;
    bvh.prim_index = tree.order;                               // the object arrays of engine BVH, in the reference's order
    if (env.debug_bvh)
      std::fprintf(stderr, "amber_hip: reference BVH of %u objects: %u inner nodes, %u leaves (largest %u objects), depth %u\n", s->n_objects, tree.n_inner, tree.n_leaves, tree.largest_leaf, tree.depth);
  }
  amber_filter::FilterProgram fprog;
  float fp_center[3] = {0, 0, 0}, fp_reach = 0;
  {
    // model box of the two-phase filter: bounds of every object and of the lens, doubled
    double lo[3] = {L.origin[0], L.origin[1], L.origin[2]}, hi[3] = {L.origin[0], L.origin[1], L.origin[2]};
    for (const DevObject& ob : objs) {
      const amber_bvh::Box bx = amber_bvh::ObjectBox(ob);
      for (int c = 0; c < 3; c++) { lo[c] = std::min<double>(lo[c], bx.mn[c]); hi[c] = std::max<double>(hi[c], bx.mx[c]); }
    }
    double reach = 0;
    for (int c = 0; c < 3; c++) { fp_center[c] = static_cast<float>(0.5 * (lo[c] + hi[c])); reach = std::max(reach, 0.5 * (hi[c] - lo[c])); }
    fp_reach = static_cast<float>(std::min(3.0e38, 2.0 * reach + 1e-3));
  }
  DeriveLens(L, s->objects + L.first_blade_object, *sensor, fp_center, fp_reach, p.lens, blades, p.aperture_rect);   // (the blades' slots follow below)
  std::vector<amber_filter::FilterProgram> more_progs;          // engine TWO_PHASE_N: the programs of groups 1, 2, ... (fprog is group 0's)
  if (p.hit_engine == kHitTwoPhaseN) {
    // groups of 32 in scene order, the aperture blades first (the primary rounds' masks and the blades' own slots live in group 0)
    std::vector<uint32_t> order;
    for (uint32_t i = 0; i < L.n_blades; i++) order.push_back(L.first_blade_object + i);
    for (uint32_t i = 0; i < s->n_objects; i++) if (i < L.first_blade_object || i >= L.first_blade_object + L.n_blades) order.push_back(i);
    for (size_t first = 0; first < order.size(); first += 32) {
      const std::vector<uint32_t> members(order.begin() + first, order.begin() + std::min(order.size(), first + 32));
      if (first == 0) amber_filter::BuildFilterProgram(objs, fp_center, fprog, &members);
      else { more_progs.emplace_back(); amber_filter::BuildFilterProgram(objs, fp_center, more_progs.back(), &members); }
    }
  } else if (p.two_phase) amber_filter::BuildFilterProgram(objs, fp_center, fprog);
  if (p.two_phase && env.debug_filter) {     // diagnostic: shape of the Phase-A program
    uint32_t pairs = 0, singles = 0;
    uint32_t shared = 0;
    for (const DevPlane& pl : fprog.planes) { pairs += pl.n_pairs; singles += pl.n_tris & 0x7fffffffu; shared += pl.n_tris >> 31; }
    std::fprintf(stderr, "amber_hip: filter program%s: %zu planes (%u share the previous plane's normal), %u pair records, %u single records, %zu spheres, always mask %#x; %zu group(s) of <= 32 objects\n",
                 more_progs.empty() ? "" : " of group 0", fprog.planes.size(), shared, pairs, singles, fprog.spheres.size(), fprog.always_mask, more_progs.size() + 1);
  }
  p.prog_order = fprog.order;
  p.host_planes = fprog.planes;
  for (uint32_t i = 0; i < L.n_blades; i++)            // filter-program slot of every aperture blade (self-candidate trip)
    for (uint32_t k = 0; k < fprog.n_prog_tris; k++)
      if (fprog.order[k] == L.first_blade_object + i) blades[i].slot = static_cast<int32_t>(k);
  p.lights.resize(s->n_lights);
  for (uint32_t i = 0; i < s->n_lights; i++) {
    const AmberFlatLight& fl = s->lights[i];
    const AmberFlatObject& fo = s->objects[fl.object];
    DevLight& dl = p.lights[i];
    std::memset(&dl, 0, sizeof dl);
    dl.kind = fo.kind; dl.slot = -1; dl.cum_power = fl.cum_power; dl.pdf_area = fl.pdf_area;
    for (int c = 0; c < 3; c++) dl.irr[c] = fl.irradiance[c];
    for (int c = 0; c < 12; c++) dl.p[c] = fo.p[c];
    for (uint32_t k = 0; k < fprog.n_prog_tris; k++)
      if (fprog.order[k] == fl.object) dl.slot = static_cast<int32_t>(k);
    for (size_t g = 0; g < more_progs.size(); g++)              // LDS slots of group g + 1 start at 32 (g + 1)
      for (uint32_t k = 0; k < more_progs[g].n_prog_tris; k++)
        if (more_progs[g].order[k] == fl.object) dl.slot = static_cast<int32_t>(32u * (g + 1) + k);
  }
  // every group's records behind each other; the LDS image: 32 slots per group, kind |= scene index << 8 | 0x80 for a filtered triangle
  p.planes = fprog.planes;
  p.tri_filters = fprog.tris;
  p.sphere_filters = fprog.spheres;
  std::vector<DevObject>& prog = p.prog_objects;
  prog.resize(more_progs.empty() ? fprog.order.size() : 32u * (more_progs.size() + 1));
  if (!prog.empty()) std::memset(prog.data(), 0, prog.size() * sizeof(DevObject));
  auto place = [&](const amber_filter::FilterProgram& fp, size_t base) {
    for (size_t k = 0; k < fp.order.size(); k++) { prog[base + k] = objs[fp.order[k]]; prog[base + k].kind |= fp.order[k] << 8 | (!more_progs.empty() && k < fp.n_prog_tris ? 0x80u : 0u); }   // (the flag only in the grouped engine's image)
  };
  place(fprog, 0);
  if (more_progs.empty()) amber_filter::MarkFlatSelf(prog, fprog.n_prog_tris);   // the 32-object engine only: its axis-flat program triangles (filter_build.h, "Flat self")
  if (!more_progs.empty()) {
    auto record = [&](const amber_filter::FilterProgram& fp, size_t plane_first, size_t tri_first, size_t sphere_first) {
      DevFilterGroup g{};
      g.plane_first = static_cast<uint32_t>(plane_first); g.n_planes = static_cast<uint32_t>(fp.planes.size()); g.slab_ends = amber_filter::SlabEnds(fp);
      g.tri_first = static_cast<uint32_t>(tri_first); g.sphere_first = static_cast<uint32_t>(sphere_first); g.n_sphere_filters = static_cast<uint32_t>(fp.spheres.size());
      g.always_mask = fp.always_mask; g.n_prog_tris = fp.n_prog_tris; g.n_objects = static_cast<uint32_t>(fp.order.size());
      p.groups.push_back(g);
    };
    record(fprog, 0, 0, 0);
    for (size_t g = 0; g < more_progs.size(); g++) {
      const amber_filter::FilterProgram& fp = more_progs[g];
      record(fp, p.planes.size(), p.tri_filters.size(), p.sphere_filters.size());
      p.planes.insert(p.planes.end(), fp.planes.begin(), fp.planes.end());
      p.tri_filters.insert(p.tri_filters.end(), fp.tris.begin(), fp.tris.end());
      p.sphere_filters.insert(p.sphere_filters.end(), fp.spheres.begin(), fp.spheres.end());
      place(fp, 32u * (g + 1));
    }
  }

  if (!p.bvh_pending) FillBvhArrays(p, p, objs, bvh);
  p.ref_nodes = std::move(ref_tree.nodes);
  p.ref_leaves = std::move(ref_tree.leaves);

  DevScene& sc = p.scene;
  sc.n_planes = static_cast<uint32_t>(fprog.planes.size()); sc.slab_ends = amber_filter::SlabEnds(fprog); sc.n_sphere_filters = static_cast<uint32_t>(fprog.spheres.size());
  if (p.hit_engine == AMBER_ENGINE_REFERENCE_BVH) sc.bvh_root = ref_tree.root;
  for (int c = 0; c < 3; c++) sc.fp_center[c] = fp_center[c];
  sc.fp_reach = fp_reach;
  // origin within fp_reach (max norm) of the centre, objects within half of that: no two such points are farther apart than
  sc.fp_tmax = static_cast<float>(std::min(3.0e38, 1.7320508 * 1.5 * 1.01 * static_cast<double>(fp_reach)));
  sc.n_lights = s->n_lights; sc.total_power = s->n_lights ? s->lights[s->n_lights - 1].cum_power : 0.0f;
  sc.n_prog_tris = fprog.n_prog_tris; sc.always_mask = fprog.always_mask;
  sc.n_groups = static_cast<uint32_t>(p.groups.empty() ? 1 : p.groups.size()); sc.n_lds_objects = static_cast<uint32_t>(prog.size());
  sc.blade_mask = 0u;
  for (const DevBlade& bl : blades) if (bl.slot >= 0 && bl.slot < 32) sc.blade_mask |= 1u << bl.slot;
  sc.n_objects = s->n_objects; sc.max_depth = params->max_depth;
  sc.sensor.w = sensor->width; sc.sensor.h = sensor->height;
  sc.sensor.wf = static_cast<float>(sensor->width); sc.sensor.hf = static_cast<float>(sensor->height);
  sc.sensor.sw = sensor->scene_width; sc.sensor.sh = sensor->scene_height;
  sc.sensor.size_f = static_cast<float>(static_cast<uint64_t>(sensor->width) * sensor->height);
  return p;
}

}  // namespace amber_prep

// bvh_update.inc -- amber_hip_pt_update_objects: new geometry for the objects of a live handle, and engine BVH's tree made valid again on the
// device; amber_hip_pt_update_lens: the same for the aperture blades, with the lens they belong to (UpdateLens, at the end).  Part of the one translation unit pt_host.hip; uses the kernels and the scratch of bvh_device_build.inc.
//
// An update is always a pass over the WHOLE scene: the sphere slack 16 eps D^2 and the needle reach depend on the scene diagonal, so when one
// object moves the widened box of every object may change, and the binary16 grid changes with the bounds, so every plane word changes.  Only
// the upload is proportional to the number of objects replaced.
//
// Order of work (all or nothing: until step 4 nothing the render kernels read has been touched):
//   1  the resident object array is copied to the handle's second array; bu_convert writes the new records over their range of it -- the
//      arithmetic of PrepareScene's flatten loop -- and records the first object whose kind or material differs from the resident one
//   2  db_bounds_raw, db_bounds_wide over the second array (REBUILD: the whole of DeviceBuildBvh's first half)
//   3  one read-back: bounds, smallest sphere radius, the error word (REBUILD: depth and node count too); refused -> return, handle unchanged
//   4  REFIT: bu_parents (once per topology), bu_refit (leaf boxes, bottom-up unions), bu_emit (PadBox, PlaneWordOutward: the plane words of
//      every node, child references untouched), db_gather through the leaf order the tree keeps.  REBUILD: db_emit, db_gather into the handle's arrays.
//   5  the two object arrays change places; bu_area; the call waits for the stream a second and last time.
// A HIP runtime failure after step 3 (AMBER_EHIP) may leave step 4 half enqueued: such a handle is to be destroyed.
//
// bu_refit hands boxes between workgroups by db_boxes' protocol: a thread per leaf reference walks towards the root, at every node the SECOND
// arrival continues with the union; every handed-over word is an agent-scope atomic store / load around an agent-scope acq_rel counter.  A
// carried box never holds a NaN (reset, then grow), so the unions are a function of the scene alone, never of the arrival order.

namespace {
int ResolvePending(amber_hip_pt* h);                          // pt_launch.inc

namespace dupd {

using amber_bvh::Box;
using dbuild::kNoParent;

// PrepareScene's flatten loop for the objects [first, first + count): the library is compiled with -ffp-contract=off, E1 and E2 are single
// binary32 subtractions.  A record may only replace one of its own kind and material.
__global__ void __launch_bounds__(256) bu_convert(const AmberFlatObject* __restrict__ flat, uint32_t first, uint32_t count, const DevObject* __restrict__ resident,
                                                  DevObject* __restrict__ out, uint32_t n, dbuild::Reduced* r) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= count || first + i >= n) return;
  const AmberFlatObject f = flat[i];
  DevObject o = {};
  o.kind = f.kind; o.material = f.material;
  o.a[0] = f.p[0]; o.a[1] = f.p[1]; o.a[2] = f.p[2];
  if (f.kind == AMBER_PRIM_TRIANGLE) {
    for (int c = 0; c < 3; c++) { o.e1[c] = f.p[3 + c] - f.p[c]; o.e2[c] = f.p[6 + c] - f.p[c]; o.n[c] = f.p[9 + c]; }
  } else if (f.kind == AMBER_PRIM_SPHERE) {
    o.radius = f.p[3];
  } else {
    o.e1[0] = f.p[3]; o.e1[1] = f.p[4]; o.e1[2] = f.p[5]; o.radius = f.p[6]; o.height = f.p[7];
  }
  const DevObject old = resident[first + i];
  if (f.kind != (old.kind & 0xffu) || f.material != old.material) atomicMin(&r->bad_index, first + i);
  out[first + i] = o;
}

// parent[child] = node * 2 + side for every inner child (the array has been filled with kNoParent: the root keeps it)
__global__ void __launch_bounds__(256) bu_parents(const DevBvhNodeQ* __restrict__ nodes, uint32_t n_nodes, uint32_t* __restrict__ parent) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_nodes) return;
  const int32_t l = nodes[i].left, r = nodes[i].right;
  if (l >= 0 && static_cast<uint32_t>(l) < n_nodes) parent[l] = 2u * i;
  if (r >= 0 && static_cast<uint32_t>(r) < n_nodes) parent[r] = 2u * i + 1u;
}

// One thread per child reference; those that name a leaf compute its box -- reset, then grown by the widened boxes of its (at most three)
// leaf-order slots -- and walk towards the root.  child_boxes: [node][side][8] words {mn[3], mx[3], -, -}; arrivals: [node], zero.
__global__ void __launch_bounds__(256) bu_refit(const DevBvhNodeQ* __restrict__ nodes, uint32_t n_nodes, const uint32_t* __restrict__ prims, uint32_t n,
                                                const Box* __restrict__ boxes, const uint32_t* __restrict__ parent, uint32_t* child_boxes, uint32_t* arrivals) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= 2u * n_nodes) return;
  uint32_t node = t >> 1, side = t & 1u;
  const int32_t ref = side ? nodes[node].right : nodes[node].left;
  if (ref >= 0) return;
  const uint32_t leaf = static_cast<uint32_t>(-(ref + 1)), first = leaf >> 4, count = leaf & 3u;
  Box b; b.reset();
  for (uint32_t k = 0; k < count; k++) {
    if (first + k >= n) break;
    const uint32_t object = prims[first + k];
    if (object < n) b.grow(boxes[object]);
  }
  for (uint32_t level = 0; level < 64u; level++) {             // (no tree in use is deeper than kMaxDepth)
    uint32_t* mine = child_boxes + (static_cast<size_t>(node) * 2u + side) * 8u;
    for (int c = 0; c < 3; c++) { dbuild::PublishWord(mine + c, __float_as_uint(b.mn[c])); dbuild::PublishWord(mine + 3 + c, __float_as_uint(b.mx[c])); }
    const uint32_t before = __hip_atomic_fetch_add((dbuild::GlobalWord*)(arrivals + node), 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (before == 0u) return;                                  // the sibling subtree is not finished: its last thread will continue from here
    uint32_t* theirs = child_boxes + (static_cast<size_t>(node) * 2u + (side ^ 1u)) * 8u;
    Box o;
    for (int c = 0; c < 3; c++) { o.mn[c] = __uint_as_float(dbuild::ConsumeWord(theirs + c)); o.mx[c] = __uint_as_float(dbuild::ConsumeWord(theirs + 3 + c)); }
    b.grow(o);
    const uint32_t up = parent[node];
    if (up == kNoParent || (up >> 1) >= n_nodes) return;       // the root
    node = up >> 1; side = up & 1u;
  }
}

// The plane words of every node from the boxes bu_refit left (plain loads: written by an earlier launch); child references untouched
__global__ void __launch_bounds__(256) bu_emit(DevBvhNodeQ* __restrict__ nodes, uint32_t n_nodes, const uint32_t* __restrict__ child_boxes, dbuild::Grid g) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_nodes) return;
  for (uint32_t side = 0; side < 2u; side++) {
    const uint32_t* w = child_boxes + (static_cast<size_t>(i) * 2u + side) * 8u;
    Box b;
    for (int c = 0; c < 3; c++) { b.mn[c] = __uint_as_float(w[c]); b.mx[c] = __uint_as_float(w[3 + c]); }
    // a subtree of objects without bounds (NaN parameters: no ray hits them) keeps the box of reset(): no ray enters, and no plane outside the grid
    const bool empty = b.mn[0] > b.mx[0] || b.mn[1] > b.mx[1] || b.mn[2] > b.mx[2];
    amber_bvh::PadBox(b, g.extent);
    for (int c = 0; c < 3; c++) nodes[i].w[3 * side + c] = empty ? amber_bvh::EmptyPlaneWord() : amber_bvh::PlaneWordOutward(b.mn[c], b.mx[c], g.gmin[c], g.step[c]);
  }
}

// Tree quality as AmberUpdateInfo reports it, from the planes the traversal reads: out[0] += surface areas of both child boxes of every
// node, out[1] = surface area of the root (the union of its two).  The sum's rounding depends on the arrival order: informative only.
// The planes are decoded in binary64 (gmin + value * step rounds once, by 2^-53): narrowed to binary32 they lose up to half an ulp of the
// COORDINATE each, which for a thin box far from the origin (a planar mesh at z = 1234.5: boxes 0.04 thick) is 1e-3 of its side and moved
// the figure by 1e-4 (tests/test_tree_tightness.py).
__device__ __forceinline__ double PlaneBoxArea(const double lo[3], const double hi[3]) {
  const double x = hi[0] - lo[0], y = hi[1] - lo[1], z = hi[2] - lo[2];
  return (x < 0 || y < 0 || z < 0) ? 0.0 : 2.0 * (x * y + y * z + z * x);
}
__global__ void __launch_bounds__(256) bu_area(const DevBvhNodeQ* __restrict__ nodes, uint32_t n_nodes, uint32_t root, dbuild::Grid g, double* out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  double sum = 0.0;
  if (i < n_nodes) {
    double lo[2][3], hi[2][3];
    for (int side = 0; side < 2; side++)
      for (int c = 0; c < 3; c++) {
        const uint32_t w = nodes[i].w[3 * side + c];
        lo[side][c] = double(g.gmin[c]) + amber_bvh::F16Value(static_cast<uint16_t>(w & 0xffffu)) * double(g.step[c]);
        hi[side][c] = double(g.gmin[c]) + amber_bvh::F16Value(static_cast<uint16_t>(w >> 16)) * double(g.step[c]);
      }
    sum = PlaneBoxArea(lo[0], hi[0]) + PlaneBoxArea(lo[1], hi[1]);
    if (i == root) {
      double ulo[3], uhi[3];
      for (int c = 0; c < 3; c++) { ulo[c] = fmin(lo[0][c], lo[1][c]); uhi[c] = fmax(hi[0][c], hi[1][c]); }
      out[1] = PlaneBoxArea(ulo, uhi);
    }
  }
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if ((threadIdx.x & 63u) == 0u && sum != 0.0) atomicAdd(out, sum);
}

// parameters of a flat record that its kind reads
inline uint32_t ParamsOfKind(uint32_t kind) { return kind == AMBER_PRIM_TRIANGLE ? 12u : kind == AMBER_PRIM_SPHERE ? 4u : kind == AMBER_PRIM_DISK ? 7u : 8u; }

// Enqueues the measurement of the tree in use into h->area_host[2 * slot ..]: sum of child areas and root area (zeros for a scene that is one
// leaf).  No wait: AreaOf reads the figures once the stream has been waited for.
int QueueArea(amber_hip_pt* h, int slot) {
  const uint32_t n_nodes = h->build.n_nodes;
  h->area_host[2 * slot] = h->area_host[2 * slot + 1] = 0.0;
  if (n_nodes == 0u || h->scene.bvh_root < 0) return AMBER_OK;
  BvhBuildScratch& s = h->update_scratch;
  HIP_TRY(s.area.need(4));
  dbuild::Grid g{};
  for (int c = 0; c < 3; c++) { g.gmin[c] = h->scene.bvh_gmin[c]; g.step[c] = h->scene.bvh_step[c]; }
  HIP_TRY(hipMemsetAsync(s.area.p + 2 * slot, 0, 2 * sizeof(double), h->stream));
  hipLaunchKernelGGL(bu_area, dim3((n_nodes + 255u) / 256u), dim3(256), 0, h->stream, const_cast<const DevBvhNodeQ*>(h->scene.bvh_nodes), n_nodes,
                     static_cast<uint32_t>(h->scene.bvh_root), g, s.area.p + 2 * slot);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h->area_host + 2 * slot, s.area.p + 2 * slot, 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return AMBER_OK;
}
inline float AreaOf(const amber_hip_pt* h, int slot) { return h->area_host[2 * slot + 1] > 0 ? static_cast<float>(h->area_host[2 * slot] / h->area_host[2 * slot + 1]) : 0.f; }

// Steps 4 of the refit: the handle's tree over the objects at `objs`, whose widened boxes are in the scratch and whose bounds are bmn / bmx
int RefitTree(amber_hip_pt* h, const DevObject* objs, const float bmn[3], const float bmx[3], float rmin) {
  BvhBuildScratch& s = h->update_scratch;
  DevScene& sc = h->scene;
  const hipStream_t st = h->stream;
  const uint32_t n = sc.n_objects, n_nodes = h->build.n_nodes;
  const bool tree = n_nodes != 0u && sc.bvh_root >= 0;
  DevBvhNodeQ* nodes = reinterpret_cast<DevBvhNodeQ*>(h->tree.nodes.p);
  if (tree) {
    HIP_TRY(s.refit_parent.need(n_nodes)); HIP_TRY(s.child_boxes.need(static_cast<size_t>(n_nodes) * 16u)); HIP_TRY(s.arrivals.need(n_nodes));
  }
  const dbuild::Grid g = dbuild::GridOfBounds(bmn, bmx, tree, sc);
  amber_prep::SetBvhRayMargin(sc, bmn, bmx, h->has_spheres, h->has_spheres ? rmin : 0.0f);
  if (tree) {
    const dim3 by_node((n_nodes + 255u) / 256u), by_ref((2u * n_nodes + 255u) / 256u), wg(256);
    if (!s.refit_parent_valid) {
      HIP_TRY(hipMemsetAsync(s.refit_parent.p, 0xff, static_cast<size_t>(n_nodes) * sizeof(uint32_t), st));
      hipLaunchKernelGGL(bu_parents, by_node, wg, 0, st, const_cast<const DevBvhNodeQ*>(nodes), n_nodes, s.refit_parent.p);
      s.refit_parent_valid = true;
    }
    HIP_TRY(hipMemsetAsync(s.arrivals.p, 0, static_cast<size_t>(n_nodes) * sizeof(uint32_t), st));
    hipLaunchKernelGGL(bu_refit, by_ref, wg, 0, st, const_cast<const DevBvhNodeQ*>(nodes), n_nodes, sc.bvh_prims, n, s.boxes.p, s.refit_parent.p, s.child_boxes.p, s.arrivals.p);
    hipLaunchKernelGGL(bu_emit, by_node, wg, 0, st, nodes, n_nodes, s.child_boxes.p, g);
  }
  hipLaunchKernelGGL(dbuild::db_gather, dim3((n + 255u) / 256u), dim3(256), 0, st, objs, sc.bvh_prims, n, static_cast<uint32_t*>(nullptr),
                     reinterpret_cast<DevObject*>(h->tree.objects.p), reinterpret_cast<float4*>(h->tree.spheres.p),
                     h->n_triangles != 0 ? reinterpret_cast<float4*>(h->tree.tris.p) : nullptr);
  HIP_TRY(hipGetLastError());
  return AMBER_OK;
}

}  // namespace dupd

// amber_hip_pt_update_lens: what the handle's lens becomes at the commit point of the update that carries its blade records
struct LensChange {
  DevLens lens;
  std::vector<DevBlade> blades;
  float aperture_rect[4][3];
};
constexpr size_t kLensBladesOffset = (sizeof(DevLens) + 15u) / 16u * 16u;

// amber_hip_pt_update_objects (lens_change == nullptr), and amber_hip_pt_update_lens: the same update with the blade records as the changed objects
// and the new lens swapped in at the same commit point.  t0: when the public call began (update_ms).
int UpdateScene(amber_hip_pt* h, uint32_t first, uint32_t count, const AmberFlatObject* objects, uint32_t mode, AmberUpdateInfo* info,
                const LensChange* lens_change, const std::string& who, std::chrono::steady_clock::time_point t0) {
  using namespace dupd;
  if (mode != AMBER_UPDATE_REFIT && mode != AMBER_UPDATE_REBUILD) return Fail(AMBER_EINVAL, who + ": unknown mode " + std::to_string(mode));
#if AMBER_BVH_WIDE
  return Fail(AMBER_EINVAL, who + ": not in an AMBER_BVH_WIDE measurement build (the device writes 2-wide nodes only): re-create the handle");
#endif
  if (h->hit_engine != AMBER_ENGINE_BVH || h->engine == AMBER_ENGINE_WAVEFRONT)
    return Fail(AMBER_EINVAL, who + ": only engine BVH's tree is updated on the device (AUTO past 80 objects, AMBER_ENGINE_BVH); with this "
                              "handle's engine a create costs no more than an update would: re-create the handle");
  DevScene& sc = h->scene;
  const uint32_t n = sc.n_objects;
  if (first > n || count > n - first) return Fail(AMBER_EINVAL, who + ": objects [" + std::to_string(first) + ", " + std::to_string(uint64_t(first) + count) +
                                                                ") are not all in the scene (" + std::to_string(n) + " objects)");
  if (count && !objects) return Fail(AMBER_EINVAL, who + ": null objects");
  auto fill = [&](uint32_t mode_used, uint32_t reason, float before) {
    if (!info) return;
    info->mode_used = mode_used; info->fallback_reason = reason; info->n_nodes = h->build.n_nodes; info->depth = h->build.depth;
    info->area_before = before; info->area_after = h->tree_area;
    info->update_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };
  if (count == 0) {                                            // nothing changes; the figures are those of the tree in use
    if (!h->area_known) {
      HIP_TRY(hipSetDevice(h->device));
      AMBER_TRY(QueueArea(h, 0));
      HIP_TRY(hipStreamSynchronize(h->stream));
      h->tree_area = AreaOf(h, 0); h->area_known = true;
    }
    fill(mode, AMBER_BUILD_REASON_NONE, h->tree_area);
    return AMBER_OK;
  }

  // the aperture blades stay what they are unless their lens comes with them (lens, DevBlade and p_area derive from them); does a light's object change?
  const uint32_t n_blades = lens_change ? 0u : static_cast<uint32_t>(h->blade_records.size());
  for (uint32_t b = 0; b < n_blades; b++) {
    const uint32_t i = h->first_blade + b;
    if (i - first < count && std::memcmp(&objects[i - first], &h->blade_records[b], sizeof(AmberFlatObject)) != 0)
      return Fail(AMBER_EINVAL, who + ": object " + std::to_string(i) + " is an aperture blade and its record differs from the resident one (the lens and its blades change through amber_hip_pt_update_lens)");
  }
  bool lights_change = false;
  for (size_t l = 0; l < h->light_object.size() && !lights_change; l++) {
    const uint32_t i = h->light_object[l];
    if (i - first < count) lights_change = std::memcmp(objects[i - first].p, &h->light_p[12 * l], ParamsOfKind(objects[i - first].kind) * sizeof(float)) != 0;
  }

  HIP_TRY(hipSetDevice(h->device));
  AMBER_TRY(ResolvePending(h));   // a pass enqueued before this call renders the old scene, also when the host has to repeat it
  const hipStream_t st = h->stream;
  BvhBuildScratch& s = h->update_scratch;
  const bool measure_before = !h->area_known;                  // a handle's first update: the figure comes with the bounds' read-back
  if (measure_before) AMBER_TRY(QueueArea(h, 0));
  const size_t object_bytes = static_cast<size_t>(n) * sizeof(DevObject);
  HIP_TRY(h->objects_alt.need(object_bytes)); HIP_TRY(s.staged.need(count)); HIP_TRY(s.red.need(1)); HIP_TRY(s.boxes.need(n));
  DevObject* fresh = reinterpret_cast<DevObject*>(h->objects_alt.p);

  // 1: the new scene's records
  if (count < n) HIP_TRY(hipMemcpyAsync(fresh, sc.objects, object_bytes, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(s.staged.p, objects, static_cast<size_t>(count) * sizeof(AmberFlatObject), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(dbuild::db_init, dim3(1), dim3(64), 0, st, s.red.p);
  hipLaunchKernelGGL(bu_convert, dim3((count + 255u) / 256u), dim3(256), 0, st, const_cast<const AmberFlatObject*>(s.staged.p), first, count, sc.objects, fresh, n, s.red.p);
  HIP_TRY(hipGetLastError());
  uint8_t* fresh_lens = nullptr;                               // ... and the new lens and blades, into the buffer no enqueued pass reads
  if (lens_change) {
    const size_t blade_bytes = lens_change->blades.size() * sizeof(DevBlade);
    DevBuf<uint8_t>& buf = h->lens_alt[h->lens_alt_next];
    HIP_TRY(buf.need(kLensBladesOffset + blade_bytes));
    h->lens_stage.assign(kLensBladesOffset + blade_bytes, 0);
    std::memcpy(h->lens_stage.data(), &lens_change->lens, sizeof(DevLens));
    std::memcpy(h->lens_stage.data() + kLensBladesOffset, lens_change->blades.data(), blade_bytes);
    HIP_TRY(hipMemcpyAsync(buf.p, h->lens_stage.data(), h->lens_stage.size(), hipMemcpyHostToDevice, st));
    fresh_lens = buf.p;
  }

  const DevScene saved = sc;                                   // (restored on every refusal below: all or nothing)
  const auto refused = [&](const dbuild::Reduced& red) -> int {
    sc = saved;
    if (red.bad_index != kNoParent)
      return Fail(AMBER_EINVAL, who + ": object " + std::to_string(red.bad_index) + ": kind or material differs from the resident record's (an update moves geometry only)");
    return Fail(AMBER_EINVAL, who + ": the new scene has no finite bounds");
  };
  uint32_t mode_used = mode, reason = AMBER_BUILD_REASON_NONE;
  dbuild::Reduced red;
  bool bounds_known = false;
  if (mode == AMBER_UPDATE_REBUILD) {
    dbuild::BuildInput in{};
    in.objs = fresh; in.n = n; in.any_tri = h->n_triangles != 0; in.has_spheres = h->has_spheres; in.rmin_known = false; in.prepared = true;
    for (int k = 0; k < 3; k++) in.small_kinds[k] = h->small_kinds[k];
    dbuild::BuildResult res{};
    const int rc = DeviceBuildBvh(h, in, s, &res);
    if (rc != AMBER_OK) { sc = saved; return rc; }
    red = res.red; bounds_known = true;
    if (res.reason == dbuild::kReasonRejected || res.reason == AMBER_BUILD_REASON_BOUNDS) return refused(red);
    if (res.reason == AMBER_BUILD_REASON_NONE) {
      s.refit_parent_valid = false;
      amber_prep::ChooseBvhScheduler(*h, n, h->n_triangles, h->create_flags, h->env, res.n_nodes, res.depth, AMBER_PATH_BVH_STACK, AMBER_BVH_SHADE_BATCH);
      h->build.where = AMBER_BUILD_DEVICE; h->build.fallback_reason = AMBER_BUILD_REASON_NONE;
      h->build.n_nodes = res.n_nodes; h->build.n_leaves = res.n_nodes + 1u; h->build.depth = res.depth;
    } else {                                                   // the Morton tree is too deep to walk: the topology in use is always valid
      mode_used = AMBER_UPDATE_REFIT; reason = res.reason;
    }
  }
  if (mode_used == AMBER_UPDATE_REFIT) {
    if (!bounds_known) {
      double slack_factor = 16.0;
      if (const char* env = std::getenv("AMBER_BVH_SPHERE_SLACK")) slack_factor = std::atof(env);   // BuildBvh's test hook
      const dim3 by_object((n + 255u) / 256u), wg(256);
      hipLaunchKernelGGL(dbuild::db_bounds_raw, by_object, wg, 0, st, const_cast<const DevObject*>(fresh), n, s.red.p);
      hipLaunchKernelGGL(dbuild::db_bounds_wide, by_object, wg, 0, st, const_cast<const DevObject*>(fresh), n, s.red.p, slack_factor, s.boxes.p);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(&red, s.red.p, sizeof red, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
    float bmn[3], bmx[3];
    if (red.bad_index != kNoParent || !dbuild::FiniteBounds(red, bmn, bmx)) return refused(red);
    const int rc = RefitTree(h, fresh, bmn, bmx, dbuild::KeyFloat(red.rmin));
    if (rc != AMBER_OK) { sc = saved; return rc; }
  }
  // 5: commit.  (Both paths have waited for the stream once, for the read-back: the first update's area_before is on the host.)
  const float area_before = measure_before ? AreaOf(h, 0) : h->tree_area;
  h->objects_buf.swap(h->objects_alt);
  sc.objects = fresh;
  h->lights_stale = h->lights_stale || lights_change;
  if (lens_change) {                                           // the host's readers of the lens (h->lens, aperture_rect, blade_records) see the new one from here on
    sc.lens = reinterpret_cast<const DevLens*>(fresh_lens);
    sc.blades = reinterpret_cast<const DevBlade*>(fresh_lens + kLensBladesOffset);
    h->lens_alt_next ^= 1u;
    h->lens = lens_change->lens;
    std::memcpy(h->aperture_rect, lens_change->aperture_rect, sizeof h->aperture_rect);
    h->blade_records.assign(objects, objects + count);
  }
  AMBER_TRY(QueueArea(h, 1));
  HIP_TRY(hipStreamSynchronize(st));                           // the second and last wait: the caller's records have been read, update_ms covers the work
  s.retired_nodes.reset();
  h->tree_area = AreaOf(h, 1); h->area_known = true;
  fill(mode_used, reason, area_before);
  return AMBER_OK;
}

int UpdateObjects(amber_hip_pt* h, uint32_t first, uint32_t count, const AmberFlatObject* objects, uint32_t mode, AmberUpdateInfo* info) {
  return UpdateScene(h, first, count, objects, mode, info, nullptr, "amber_hip_pt_update_objects", std::chrono::steady_clock::now());
}

// The lens of a live handle replaced: the values create derives from it come from create's own function (amber_prep::DeriveLens), the blades'
// scene objects go through the update above -- bu_convert writes them into the scene-order array, db_gather into the leaf-order arrays at the
// slots the tree uses, the whole-scene pass makes every box valid for the new bounds -- and the lens changes at that update's commit point.
int UpdateLens(amber_hip_pt* h, const AmberFlatThinLens* lens, const AmberFlatObject* blades, uint32_t mode, AmberUpdateInfo* info) {
  const auto t0 = std::chrono::steady_clock::now();
  const std::string who = "amber_hip_pt_update_lens";
  if (!lens || !blades) return Fail(AMBER_EINVAL, who + ": null lens or blades");
  if (h->hit_engine != AMBER_ENGINE_BVH || h->engine == AMBER_ENGINE_WAVEFRONT || AMBER_BVH_WIDE)   // (UpdateScene's refusals, before the lens is looked at)
    return UpdateScene(h, h->first_blade, static_cast<uint32_t>(h->blade_records.size()), blades, mode, info, nullptr, who, t0);
  const uint32_t n_blades = static_cast<uint32_t>(h->blade_records.size());
  if (lens->kind != h->lens.kind || lens->n_blades != n_blades || lens->first_blade_object != h->first_blade)
    return Fail(AMBER_EINVAL, who + ": kind " + std::to_string(lens->kind) + ", n_blades " + std::to_string(lens->n_blades) + ", first_blade_object " +
                                  std::to_string(lens->first_blade_object) + " differ from the resident lens's (" + std::to_string(h->lens.kind) + ", " + std::to_string(n_blades) +
                                  ", " + std::to_string(h->first_blade) + "): a lens update keeps them; re-create the handle");
  for (uint32_t b = 0; b < n_blades; b++)
    if (blades[b].kind != AMBER_PRIM_TRIANGLE || blades[b].material != h->blade_records[b].material)
      return Fail(AMBER_EINVAL, who + ": blade " + std::to_string(b) + " is not a triangle of the resident blade's material");
  LensChange change;
  amber_prep::DeriveLensOfState(*h, *lens, blades, change.lens, change.blades, change.aperture_rect);
  return UpdateScene(h, h->first_blade, n_blades, blades, mode, info, &change, who, t0);
}

}  // namespace

// pt_host.hip -- the ONE translation unit of the gfx950 path-tracing engine: the handle, the host side of every launch and the C ABI
// (include/amber_hip.h).  The kernels live in files of their own and are included here, where they are launched:
//   c_boundary.h           the rule of the C ABI: no exception crosses an extern "C" function -- every entry point that can allocate or form a message runs under
//                          Guarded(name, f) (bad_alloc / system_error -> AMBER_ENOMEM, anything else -> AMBER_EHIP); the thread-local message, Fail, HIP_TRY, AMBER_TRY
//   pt_args.h              RenderArgs; record emission (accumulation without owners)
//   exact_div.h            exact division by a launch constant without a divide (the pixel bookkeeping of the render kernels)
//   pt_megakernel.inc      pt_megakernel: persistent waves, work unit = ONE PATH (q = band pixel * n_samples + sample), a wave claims 1024 paths with
//                          one atomicAdd; lanes are decoupled from pixels through the wave's LDS pool; 64 fresh paths of one pixel start together
//                          (primary round, candidates from the per-pixel masks).  Engines LIST / TWO_PHASE (<= 32 objects; groups of 32 up to 128), engine BVH on trees of depth <= 12
//                          (one-shot per-lane traversal, stack in LDS), light tracing.
//   pt_bvh_megakernel.inc  pt_bvh_megakernel: engine BVH on deep trees -- lanes own (pixel, chunk of 8 samples) items, the closest hit is a RESUMABLE
//                          per-lane traversal of the 2-wide binary16-plane tree advanced in wave rounds until a batch of lanes has finished; per-item
//                          sums, reduce_partials_kernel.
//   bvh_device_build.inc   AMBER_PT_FLAG_DEVICE_BUILD: engine BVH's tree built by kernels at create (Morton order, radix-tree hierarchy, the host builder's
//                          bounds / padding / outward binary16 planes) instead of bvh_build.h's binned-SAH build on the host.
//   bvh_update.inc         amber_hip_pt_update_objects: new object geometry into a live handle -- records converted and checked by a kernel, then the
//                          tree made valid again on the device: refitted (any tree, topology kept) or rebuilt (the Morton tree, in place).
//   ray_query.inc          amber_hip_pt_cast_rays / amber_hip_pt_occluded: the caller's rays through the handle's engine -- engine BVH in a persistent refill
//                          kernel (closest hit, and the any-hit walk BvhAnyHit), the other engines one thread per ray through ClosestHit<kEngine>;
//                          LaunchPerItem, the launch of every kernel with a thread per item (its engine front end: dev_closest_hit.h).
//   image_stage.inc        what the five files below share, the stage that runs on the band after accumulation: BandPixels, the zero-on-first-use band
//                          buffer (AOV sums, moments, history) with its clear / download / device pointer, the check of the output arguments and the
//                          output tail, the check of the filters' parameters, the device helpers of the filters' kernels (stops, luminance, guide record).
//   resolve.inc            amber_hip_pt_resolve: the framebuffer's sums as the mean or, through Filmic + Gamma, as 8-bit RGB / RGBA, in device memory --
//                          a streaming kernel, four output pixels per thread, bytes equal to the host's output stage.
//   aov.inc                amber_hip_pt_aov_pass and its three companions: the first-hit guide images (albedo, depth, normal, coverage) of the band --
//                          one thread per band pixel looping over the samples, the eight sums in registers, every engine's own closest hit.
//   denoise.inc            amber_hip_pt_denoise: the edge-avoiding a-trous filter of the mean image guided by the AOV buffer -- a prepare kernel (mean and
//                          guide records), one kernel per level (a thread per pixel, 25 taps, polynomial edge stops), then resolve.inc's kernel.
//   denoise_variance.inc   amber_hip_pt_render_batch's fold and the moments buffer's three companions, and amber_hip_pt_denoise_variance: the same filter with a
//                          luminance stop scaled by the per-pixel variance of the mean, colour and variance in one 16-byte record per pixel.
//   temporal.inc           amber_hip_pt_temporal and its three companions: a per-pixel history of the mean image -- one kernel reprojects the previous history
//                          through the previous lens, validates it against the previous guide records, blends and writes; then denoise.inc's levels.
//   lt_accumulate.inc      amber_hip_lt_render_pass: the splat records of a light-tracing launch into the framebuffer in the reference's order -- an index
//                          permutation sorted by (pixel, pass, path, bounce) with two stable radix sorts, then one thread per pixel run.
//   pt_records.inc         records {q, rgb} -> path order -> the per-pixel sums of the numerical contract (rec_rank / scan / place, reduce_flagged);
//                          pixel_mask_kernel (candidates of a pixel block's eye rays).
// LAB BUILD (-DAMBER_LAB -> libamber_hip_lab.so; include/amber_hip_lab.h): the schedulers that were measured and lost but stay provably equal
// (bvh_pool.inc, wavefront.inc, bvh_stream.inc), the known-answer kernels and entry points the tests use (lab_kernels.inc, lab_api.inc) and the
// signature instantiations of the product kernels.  libamber_hip.so is built WITHOUT it and exports only the documented ABI.
//
// Replaces: PathTracing<RGB>::Thread::operator() / Render
//           (/root/reference/src/amber/rendering/algorithm_pt.cc:112-160).
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../../include/amber_hip.h"
#ifdef AMBER_LAB
#include "../../../include/amber_hip_lab.h"
#endif
#include "c_boundary.h"
#include "pt_device.h"
#include "exact_div.h"
#include "bvh_build.h"
#include "filter_build.h"
#include "ref_bvh_build.h"

using namespace amber_dev;

namespace {

// ------------------------------------------------------------------------------------------------
// render kernel
// ------------------------------------------------------------------------------------------------
#include "pt_args.h"
#include "pt_megakernel.inc"
#include "pt_records.inc"
#include "pt_bvh_megakernel.inc"
#ifdef AMBER_LAB
#include "bvh_pool.inc"
#include "bvh_stream.inc"
#include "wavefront.inc"
#include "lab_kernels.inc"
#endif

// ------------------------------------------------------------------------------------------------
// owners of HIP resources: every allocation of a handle has one, so that deleting the handle (or an early return of create) releases it all
// ------------------------------------------------------------------------------------------------
// Device memory of n elements of T; converts to T* where the kernels' arguments and the DevScene pointers want one.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;                           // elements allocated (0: none)
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  ~DevBuf() { reset(); }
  void reset() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
  hipError_t alloc(size_t count) {        // (at least one element: no zero-size allocation)
    reset();
    const hipError_t e = hipMalloc(&p, (count ? count : 1) * sizeof(T));
    if (e != hipSuccess) p = nullptr; else n = count;
    return e;
  }
  void swap(DevBuf& o) noexcept { std::swap(p, o.p); std::swap(n, o.n); }
  // at least `count` elements, contents not kept; what the buffer held stays untouched when the allocation fails
  hipError_t need(size_t count) {
    if (p && n >= count) return hipSuccess;
    DevBuf bigger;
    const hipError_t e = bigger.alloc(count);
    if (e == hipSuccess) swap(bigger);
    return e;
  }
  operator T*() const { return p; }
};
// An event, a stream or pinned host memory, released with kRelease.
template <typename T, auto kRelease>
struct Owned {
  T v{};
  Owned() = default;
  Owned(Owned&& o) noexcept : v(o.v) { o.v = T{}; }
  ~Owned() { if (v) (void)kRelease(v); }
};
using Event = Owned<hipEvent_t, hipEventDestroy>;

}  // namespace

#include "scene_prep.h"
using amber_prep::kHitTwoPhaseN;

namespace {
namespace dbuild { struct Reduced; }
// Engine BVH's arrays on the device (DevScene.bvh_* point into them), owned by the handle by name: amber_hip_pt_update_objects rewrites them in
// place and replaces the node array when a rebuilt tree has more nodes.
struct BvhTreeBufs { DevBuf<uint8_t> nodes, prims, tris, objects, spheres; };
// Scratch of the device build (bvh_device_build.inc) and of the refit (bvh_update.inc).  Create's is local and released when create returns; a
// handle that is updated keeps one, so that an update in the steady state allocates nothing.
struct BvhBuildScratch {
  DevBuf<dbuild::Reduced> red; DevBuf<amber_bvh::Box> boxes; DevBuf<unsigned long long> codes, codes_sorted; DevBuf<uint32_t> index, sorted; DevBuf<uint8_t> temp;
  DevBuf<int32_t> left, right; DevBuf<uint32_t> first, last, parent_node, parent_object, child_boxes, arrivals, live, rank;
  DevBuf<AmberFlatObject> staged;           // update: the caller's records
  DevBuf<uint32_t> refit_parent;            // refit: parent * 2 + side of every node of the tree in use; valid while the topology stands
  bool refit_parent_valid = false;
  DevBuf<double> area;                      // update: {sum of the child boxes' areas, the root's area} of the tree before and after
  DevBuf<uint8_t> retired_nodes;            // a node array a rebuild has outgrown: passes enqueued earlier may still read it, released once the stream has been waited for
};
// amber_hip_lt_render_pass (lt_accumulate.inc): the scratch of the two sorts and of the ordered sum, grown on first use, kept, released with the handle
struct LtAccumBufs {
  DevBuf<unsigned long long> key[2];        // sort keys, in and out
  DevBuf<uint32_t> index[2];                // the permutation, in and out
  DevBuf<float4> value;                     // {rgb, pad} of the records in sorted order
  DevBuf<uint8_t> temp;                     // rocPRIM's temporary storage
  DevBuf<unsigned int> longest;             // AmberLtPassInfo.longest_run of the call in flight
  uint32_t capacity = 0;                    // records d_splats holds for that call: AMBER_LT_SPLAT_CAPACITY0, or what a launch made it grow to
#ifdef AMBER_LAB
  bool stage_timing = false;                // amber_hip_kat_lt_stage_ms: sort and sum timed with events (waits for the stream after every accumulation)
  double sort_ms = 0, sum_ms = 0;
  Event ev[3];
#endif
};
// The image stage -- everything that runs on the band after accumulation (image_stage.inc and the five files behind it): its buffers, per band pixel
struct ImageStageBufs {
  DevBuf<uint8_t> resolve_out;              // AMBER_RESOLVE_HOST: staging of the output (WriteBandOutput), grown on first use and reused
  DevBuf<float4> aov;                       // amber_hip_pt_aov_* (aov.inc): two float4, allocated and zeroed by the first call that needs them
  DevBuf<float> denoise_color[2];           // amber_hip_pt_denoise (denoise.inc): the levels' input and output, 3 floats each, grown on first use
  DevBuf<float4> denoise_guide;             // ... and the guide records {a.xyz, z} {n.xyz, rz}, two float4
  DevBuf<float4> dv_record[2];              // amber_hip_pt_denoise_variance (denoise_variance.inc): {c.rgb, var}, the levels' input and output, grown on first use
  DevBuf<float4> moments;                   // amber_hip_pt_render_batch / _moments_*: {m1, m2, batches, pad}, allocated and zeroed by the first call that needs it
  DevBuf<float4> history[2];                // amber_hip_pt_temporal (temporal.inc): {color.rgb, length} {m1, m2, 0, 0}, used ping-pong, allocated and zeroed by the first call that needs them
  DevBuf<float4> history_guide[2];          // ... and the guide records of the frame each history was written with
  uint32_t history_cur = 0;                 // the pair that holds the current history
  bool history_empty = true;                // nothing to reproject: set at create and by amber_hip_pt_temporal_reset
  DevLens history_lens{};                   // the handle's lens as the call that wrote the current history saw it
  DevBuf<float> batch;                      // amber_hip_pt_render_batch: the sums of the batch in flight, 3 floats, grown on first use
};
}  // namespace

// ------------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------------
struct amber_hip_pt : amber_prep::SceneState {   // engine, scene, lens, ...: what create prepared
  int device = 0;
  Owned<hipStream_t, hipStreamDestroy> own_stream;   // the stream create made, if any: declared first, so released after every buffer below
  hipStream_t stream = nullptr;             // the render stream: own_stream, the caller's or the legacy default stream
  amber_prep::EnvSwitches env;              // the environment switches, read once at create
  std::vector<DevBuf<uint8_t>> scene_arrays;   // the scene's arrays uploaded at create (scene.materials ... scene.lens point into them)
  DevBuf<uint8_t> objects_buf;              // scene.objects
  BvhTreeBufs tree;                         // engine BVH's arrays
  // ---- amber_hip_pt_update_objects (bvh_update.inc)
  DevBuf<uint8_t> objects_alt;              // the object array the next update fills: an update commits by exchanging it with objects_buf
  BvhBuildScratch update_scratch;
  uint32_t create_flags = 0;                // AmberPtParams.reserved
  size_t n_triangles = 0;                   // kinds never change under an update: what ChooseBvhScheduler and the leaf arrays need of them
  bool has_spheres = false;
  uint32_t small_kinds[3] = {0, 0, 0};      // kinds of a scene that is one leaf
  uint32_t first_blade = 0;
  std::vector<AmberFlatObject> blade_records;   // the aperture blades as create or the last amber_hip_pt_update_lens received them (an update of objects must leave them as they are)
  // ---- amber_hip_pt_update_lens: a DevLens and, kLensBladesOffset bytes behind it, the DevBlade array.  A lens update fills the buffer not in use
  // and commits by pointing scene.lens / scene.blades at it (create's own copies are in scene_arrays); passes enqueued before keep the old pointers
  DevBuf<uint8_t> lens_alt[2];
  uint32_t lens_alt_next = 0;
  std::vector<uint8_t> lens_stage;          // the host image of that buffer: lives until the copy has been waited for
  std::vector<uint32_t> light_object;       // object of every light, and its parameters as the lights table was computed from them
  std::vector<float> light_p;
  bool lights_stale = false;                // an update has changed an object the lights table names: light tracing needs a new handle
  bool area_known = false;
  float tree_area = 0;                      // AmberUpdateInfo.area_after of the tree in use
  double area_host[4] = {0, 0, 0, 0};       // where the two area measurements of an update are copied to
  DevBuf<uint2> d_ref_stack;                // engine REFERENCE_BVH: the traversal stack of the reference's tree, [level][thread of the largest grid]
  uint64_t ref_stack_threads = 0;           // ... and the threads it was allocated for: no launch that walks that tree may have more (CheckRefStack)
  // ---- amber_hip_pt_cast_rays / amber_hip_pt_occluded (ray_query.inc): allocated by the first query, reused by every later one
  DevBuf<int32_t> d_query_stack;            // engine BVH: the global levels of the hybrid traversal stack, [level][thread of the largest query grid]
  uint64_t query_stack_threads = 0;         // ... and the threads it was allocated for
  DevBuf<unsigned int> d_query_next;        // engine BVH: the work counter
  DevBuf<float4> d_query_rays;              // AMBER_RAYS_HOST: staging of the rays and of the results, at most kQueryStageRays rays
  DevBuf<uint8_t> d_query_out;
  ImageStageBufs img;                       // resolve, AOVs, the filters, batches
  DevBuf<float> d_fb;
  float* accum_target = nullptr;            // where reduce_flagged_kernel and reduce_partials_kernel add a pass: d_fb, except inside amber_hip_pt_render_batch (img.batch)
  DevBuf<unsigned long long> d_rays;
  DevBuf<unsigned int> d_next;
  DevBuf<unsigned long long> d_stamps;
  DevBuf<DevSplat> d_splats;
  DevBuf<unsigned int> d_splat_count;
  uint64_t hashed_seed_lt = 0;
  LtAccumBufs lt;                           // amber_hip_lt_render_pass
  DevBuf<float> d_partial;                  // pt_bvh_megakernel: per-item sums
  // path-granular accumulation (RenderPassPaths): bitmap, records in arrival order, measurements in path order, ranks
  DevBuf<uint32_t> d_flags;  bool flags_dirty = true;   // dirty: must be cleared before the next launch
  DevBuf<uint32_t> d_touched;
  DevBuf<uint4> d_records;   DevBuf<float> d_sorted;   uint32_t rec_capacity = 0;
  DevBuf<unsigned int> d_launch_ctl;        // [0] queue head of the path kernels, [1] = *d_rec_count, [2..3] = *d_rays_launch
  unsigned int* d_rec_count = nullptr;
  unsigned long long* d_rays_launch = nullptr;
  DevBuf<uint32_t> d_excl, d_block_sum;
  Owned<unsigned int*, hipHostFree> h_rec_count;   // pinned: the record counter of the launch in flight
  Event pending_event;
  bool pending = false, pending_checked = true;   // a launch whose record counter has not been looked at yet; checked = it cannot have run out of slots
  uint32_t pending_first = 0, pending_n = 0;
  float* pending_target = nullptr;          // the accumulation target of that launch: a repeat adds to the same buffer
  bool density_known = false;
  double rec_density = 0;                   // record slots used per path, as the last launch measured it
  DevBuf<int32_t> d_bvh_stack;              // pt_bvh_pool_kernel: deep traversal-stack levels
  DevBuf<float> d_carried;                  // ... and carried measurements
  DevBuf<unsigned long long> d_sig;         // amber_hip_pt_signatures
  DevBuf<uint32_t> d_pixel_mask;            // two-phase engine: primary-ray candidates per band pixel
  // pixel_mask_kernel is enqueued on the render stream by create (0.07 ms since the masks are per 4 x 4 block of pixels: it no longer pays to
  // overlap it -- a second stream costs a millisecond of host time to create, more than the kernel it would hide)
  bool pixel_mask_ready = false;            // the kernel has been enqueued in front of everything that reads d_pixel_mask
  int n_cus = 256;
  uint32_t row_begin = 0, row_end = 0, stripe_rows = 0, stripe_period = 0, local_rows = 0;
  uint64_t seed = 0, hashed_seed = 0;
  DevBuf<float> d_wf;                       // WAVEFRONT: queues + meas + counts in one allocation
  uint32_t n_materials = 0;
  std::vector<std::pair<Event, Event>> events;   // pool of event pairs, one per timed launch in flight
  size_t events_used = 0;
  uint32_t timed_launches = 0;     // launches already folded into timed_ms
  double timed_ms = 0;
};

#include "bvh_device_build.inc"
#include "bvh_update.inc"

namespace {

uint64_t HostSplitMix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int StartPixelMasks(amber_hip_pt* h, float* timing);      // defined with the launch code below
uint64_t BandPixels(const amber_hip_pt* h);               // the band's pixel count (image_stage.inc)
uint32_t PersistentBlocks(const amber_hip_pt* h, uint64_t n_items = ~0ull, bool pool = false);

int ValidateScene(const AmberFlatScene* s, const AmberSensor* sensor) {
  if (!s || !sensor) return Fail(AMBER_EINVAL, "null scene or sensor");
  if (!s->objects || s->n_objects == 0) return Fail(AMBER_EINVAL, "scene has no objects");
  if (s->n_objects >= (1u << 26)) return Fail(AMBER_EINVAL, "too many objects (engine BVH addresses its 48-byte leaf records with 32-bit byte offsets: fewer than 2^26 objects)");
  if (!s->materials || s->n_materials == 0) return Fail(AMBER_EINVAL, "scene has no materials");
  if (sensor->width == 0 || sensor->height == 0) return Fail(AMBER_EINVAL, "empty sensor");
  if (static_cast<uint64_t>(sensor->width) * sensor->height >= (1ull << 32)) return Fail(AMBER_EINVAL, "sensor too large");
  for (uint32_t i = 0; i < s->n_objects; i++) {
    if (s->objects[i].kind > AMBER_PRIM_CYLINDER) return Fail(AMBER_EINVAL, "object " + std::to_string(i) + ": unknown primitive kind");
    if (s->objects[i].material >= s->n_materials) return Fail(AMBER_EINVAL, "object " + std::to_string(i) + ": material index out of range");
  }
  for (uint32_t i = 0; i < s->n_materials; i++)
    if (s->materials[i].kind > AMBER_MAT_EYE) return Fail(AMBER_EINVAL, "material " + std::to_string(i) + ": unknown kind");
  if (s->n_lights && !s->lights) return Fail(AMBER_EINVAL, "n_lights > 0 but lights is null");
  for (uint32_t i = 0; i < s->n_lights; i++)
    if (s->lights[i].object >= s->n_objects) return Fail(AMBER_EINVAL, "light object index out of range");
  const AmberFlatThinLens& L = s->lens;
  if (L.n_blades == 0) return Fail(AMBER_EINVAL, "lens has no aperture blades");
  if (L.kind > AMBER_LENS_PINHOLE) return Fail(AMBER_EINVAL, "unknown lens kind");
  if (static_cast<uint64_t>(L.first_blade_object) + L.n_blades > s->n_objects) return Fail(AMBER_EINVAL, "aperture blade objects out of range");
  for (uint32_t i = 0; i < L.n_blades; i++)
    if (s->objects[L.first_blade_object + i].kind != AMBER_PRIM_TRIANGLE) return Fail(AMBER_EINVAL, "aperture blade is not a triangle");
  return AMBER_OK;
}


// A device copy of v, `extra` elements longer, owned by the handle; the DevScene pointer dst points to it
template <typename T, typename P>
hipError_t UploadTo(DevBuf<uint8_t>& b, const std::vector<T>& v, size_t extra, P& dst) {
  hipError_t e = b.alloc((v.size() + extra) * sizeof(T));
  if (e == hipSuccess && !v.empty()) e = hipMemcpy(b, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  if (e == hipSuccess) dst = reinterpret_cast<T*>(b.p);
  return e;
}
template <typename T, typename P>
hipError_t Upload(amber_hip_pt* h, const std::vector<T>& v, size_t extra, P& dst) {
  DevBuf<uint8_t> b;
  const hipError_t e = UploadTo(b, v, extra, dst);
  if (e == hipSuccess) h->scene_arrays.push_back(std::move(b));
  return e;
}

// validate -> prepare (scene_prep.h) -> upload (or, with AMBER_PT_FLAG_DEVICE_BUILD, build engine BVH's tree where the objects now are) -> enqueue the
// pixel masks.  Whatever the handle holds is released on every early return.
int Create(const AmberFlatScene* s, const AmberSensor* sensor, const AmberPtParams* params, amber_hip_pt** out) {
  const auto t_create = std::chrono::steady_clock::now();
  auto ms_since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
  AMBER_TRY(ValidateScene(s, sensor));
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
    return Fail(AMBER_ENODEVICE, "no HIP device available (this engine has no CPU fallback)");
  if (params->device < 0 || params->device >= n_dev) return Fail(AMBER_ENODEVICE, "device ordinal out of range");
  uint32_t rb = params->row_begin, re = params->row_end;
  if (rb == 0 && re == 0) re = sensor->height;
  // rb == re (other than 0,0) is an EMPTY band: a rank beyond the number of stripes (distributed.stripe_partition) still
  // creates a handle, whose render_pass / clear / download are no-ops, so that it can take part in the gather
  if (rb > re || re > sensor->height) return Fail(AMBER_EINVAL, "bad row band");
  uint32_t local_rows = re - rb;
  if (params->stripe_rows) {
    if (params->stripe_period < params->stripe_rows) return Fail(AMBER_EINVAL, "stripe_period must be >= stripe_rows");
    const uint32_t q = (re - rb) / params->stripe_period, rem = (re - rb) % params->stripe_period;
    local_rows = q * params->stripe_rows + (rem < params->stripe_rows ? rem : params->stripe_rows);
  }
  if (params->engine > AMBER_ENGINE_REFERENCE_BVH || params->engine == 5u) return Fail(AMBER_EINVAL, "unknown engine");
#ifndef AMBER_LAB
  if (params->engine == AMBER_ENGINE_WAVEFRONT) return Fail(AMBER_EINVAL, "engine WAVEFRONT (the streaming formulation, kept for measurement) is part of the lab build, libamber_hip_lab.so");
  if (params->reserved & AMBER_PT_FLAG_BVH_POOL) return Fail(AMBER_EINVAL, "AMBER_PT_FLAG_BVH_POOL (pt_bvh_pool_kernel, kept for measurement) is part of the lab build, libamber_hip_lab.so");
#endif
  if (params->engine == AMBER_ENGINE_REFERENCE_BVH && !amber_refbvh::CentresAreOrdered(s->objects, s->n_objects))
    return Fail(AMBER_EINVAL, "AMBER_ENGINE_REFERENCE_BVH: an object's centre is NaN (the reference's build sorts objects by centre; std::sort is undefined on NaN keys)");
  if (params->engine == AMBER_ENGINE_TWO_PHASE && s->n_objects > AMBER_MAX_GROUP_OBJECTS)
    return Fail(AMBER_EINVAL, "AMBER_ENGINE_TWO_PHASE supports at most 128 objects");

  HIP_TRY(hipSetDevice(params->device));
  const amber_prep::EnvSwitches env = amber_prep::ReadEnv();
  amber_prep::PreparedScene p = amber_prep::PrepareScene(s, sensor, params, env, AMBER_PATH_BVH_STACK, AMBER_BVH_SHADE_BATCH);
  if (!p.error.empty()) return Fail(AMBER_EINVAL, p.error);

  std::unique_ptr<amber_hip_pt, void (*)(amber_hip_pt*)> h(new amber_hip_pt(), amber_hip_pt_destroy);
  h->device = params->device;
  h->env = env;
  h->row_begin = rb; h->row_end = re; h->local_rows = local_rows;
  h->stripe_rows = params->stripe_rows; h->stripe_period = params->stripe_rows ? params->stripe_period : 0;
  h->seed = params->seed; h->hashed_seed = HostSplitMix64(params->seed);
  h->hashed_seed_lt = HostSplitMix64(params->seed + 0x6C74ull);     // light paths use streams of their own
  if (params->stream) { h->stream = static_cast<hipStream_t>(params->stream); }
  else if (params->reserved & AMBER_PT_FLAG_NULL_STREAM) { h->stream = nullptr; }     // the legacy default stream, on request
  else {
    hipError_t e = hipStreamCreateWithFlags(&h->own_stream.v, hipStreamNonBlocking);
    if (e != hipSuccess) return Fail(AMBER_EHIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    h->stream = h->own_stream.v;
  }
  static_cast<amber_prep::SceneState&>(*h) = std::move(p);      // (only the SceneState part moves: the device arrays, p.objects and p.bvh_pending stay in p
                                                                //  until the upload -- the device build and its host fallback below rely on that)
  h->n_materials = s->n_materials;
  { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, params->device) == hipSuccess && v > 0) h->n_cus = v; }

  // ---- upload (the + 1 / + 3: no array is empty on the device)
  DevScene& sc = h->scene;
  HIP_TRY(UploadTo(h->objects_buf, p.objects, 0, sc.objects));
  h->create_flags = params->reserved;
  h->n_triangles = amber_prep::CountTriangles(p.objects);
  for (size_t i = 0; i < p.objects.size(); i++) {
    h->has_spheres = h->has_spheres || (p.objects[i].kind & 0xffu) == AMBER_PRIM_SPHERE;
    if (i < 3) h->small_kinds[i] = p.objects[i].kind & 0xffu;
  }
  h->first_blade = s->lens.first_blade_object;
  h->blade_records.assign(s->objects + s->lens.first_blade_object, s->objects + s->lens.first_blade_object + s->lens.n_blades);
  for (uint32_t i = 0; i < s->n_lights; i++) {
    h->light_object.push_back(s->lights[i].object);
    h->light_p.insert(h->light_p.end(), s->objects[s->lights[i].object].p, s->objects[s->lights[i].object].p + 12);
  }
  HIP_TRY(Upload(h.get(), p.materials, 0, sc.materials));
  HIP_TRY(Upload(h.get(), p.blades, 0, sc.blades));
  HIP_TRY(Upload(h.get(), p.planes, 1, sc.planes));
  HIP_TRY(Upload(h.get(), p.tri_filters, 1, sc.tri_filters));
  HIP_TRY(Upload(h.get(), p.sphere_filters, 1, sc.sphere_filters));
  HIP_TRY(Upload(h.get(), p.prog_objects, 1, sc.prog_objects));
  if (!p.groups.empty()) HIP_TRY(Upload(h.get(), p.groups, 0, sc.groups));
  HIP_TRY(Upload(h.get(), p.lights, 1, sc.lights));
  if (p.bvh_pending) {
    // engine BVH with AMBER_PT_FLAG_DEVICE_BUILD: the tree from the objects where they now are.  A tree the traversal must not walk (too deep) or
    // that cannot be built (no finite bounds) is replaced by the host's: same arrays, same upload as without the flag.
    const auto t_tree = std::chrono::steady_clock::now();
    uint32_t reason = AMBER_BUILD_REASON_NONE, n_nodes = 0, depth = 0;
    {
      BvhBuildScratch scratch;                                   // released when this block ends
      dbuild::BuildInput in{};
      in.objs = sc.objects; in.n = static_cast<uint32_t>(p.objects.size()); in.any_tri = h->n_triangles != 0; in.has_spheres = h->has_spheres;
      in.rmin_known = true; in.rmin = 3.0e38f;
      for (const DevObject& o : p.objects) if ((o.kind & 0xffu) == AMBER_PRIM_SPHERE) in.rmin = std::min(in.rmin, std::fabs(o.radius));
      for (int k = 0; k < 3; k++) in.small_kinds[k] = h->small_kinds[k];
      dbuild::BuildResult res{};
      AMBER_TRY(DeviceBuildBvh(h.get(), in, scratch, &res));
      reason = res.reason; n_nodes = res.n_nodes; depth = res.depth;
    }
    if (reason == AMBER_BUILD_REASON_NONE) {
      amber_prep::ChooseBvhScheduler(*h, p.objects, params, env, n_nodes, depth, AMBER_PATH_BVH_STACK, AMBER_BVH_SHADE_BATCH);
      h->build.where = AMBER_BUILD_DEVICE; h->build.n_nodes = n_nodes; h->build.n_leaves = n_nodes + 1u; h->build.depth = depth;
      p.bvh_pending = false;
      h->build.tree_ms = ms_since(t_tree);
    } else {
      const double spent = ms_since(t_tree);
      amber_prep::HostBvhFallback(*h, p, reason, params, env, AMBER_PATH_BVH_STACK, AMBER_BVH_SHADE_BATCH);
      h->build.tree_ms += spent;
    }
  }
  if (h->build.where != AMBER_BUILD_DEVICE) {
    const auto t_upload = std::chrono::steady_clock::now();
    HIP_TRY(UploadTo(h->tree.nodes, p.bvh_nodes, 1, sc.bvh_nodes));
#if AMBER_BVH_WIDE
    HIP_TRY(Upload(h.get(), p.bvh_nodes4, 1, sc.bvh_nodes4));
#endif
    HIP_TRY(UploadTo(h->tree.prims, p.bvh_prims, 1, sc.bvh_prims));
    HIP_TRY(UploadTo(h->tree.tris, p.bvh_tris, 3, sc.bvh_tris));
    HIP_TRY(UploadTo(h->tree.objects, p.bvh_objects, 1, sc.bvh_objects));
    HIP_TRY(UploadTo(h->tree.spheres, p.bvh_spheres, 1, sc.bvh_spheres));
    if (h->hit_engine == AMBER_ENGINE_BVH) h->build.tree_ms += ms_since(t_upload);
  }
  HIP_TRY(Upload(h.get(), std::vector<DevLens>{p.lens}, 0, sc.lens));
  const size_t fb_floats = static_cast<size_t>(local_rows) * sensor->width * 3;
  HIP_TRY(h->d_fb.alloc(fb_floats));
  h->accum_target = h->d_fb;
  HIP_TRY(h->d_rays.alloc(1));
  HIP_TRY(h->d_next.alloc(1));
#ifdef AMBER_STAMPS
  HIP_TRY(h->d_stamps.alloc(8 + 4 * AMBER_WAVE_TIME_SLOTS));     // 8 section sums, then per wave: start, first claim done, queue empty, end
  HIP_TRY(hipMemset(h->d_stamps, 0, (8 + 4 * AMBER_WAVE_TIME_SLOTS) * sizeof(unsigned long long)));
#endif
  HIP_TRY(hipMemsetAsync(h->d_fb, 0, fb_floats * sizeof(float), h->stream));
  HIP_TRY(hipMemsetAsync(h->d_rays, 0, sizeof(unsigned long long), h->stream));
  if (h->hit_engine == AMBER_ENGINE_REFERENCE_BVH) {
    HIP_TRY(Upload(h.get(), p.ref_nodes, 1, sc.ref_nodes));
    HIP_TRY(Upload(h.get(), p.ref_leaves, 1, sc.ref_leaves));
    // one stack column per thread of the largest grid a launch of this handle uses; a walk from the root pushes at most one entry per level
    const uint64_t threads = static_cast<uint64_t>(PersistentBlocks(h.get())) * 256u;
    const uint64_t bytes = threads * (static_cast<uint64_t>(p.ref_depth) + 1u) * sizeof(uint2);
    if (bytes > (64ull << 30)) return Fail(AMBER_ENOMEM, "the reference's BVH of this scene is " + std::to_string(p.ref_depth) + " levels deep: its traversal stacks would take " + std::to_string(bytes >> 30) + " GiB");
    HIP_TRY(h->d_ref_stack.alloc(bytes / sizeof(uint2)));
    sc.ref_stack = h->d_ref_stack; sc.ref_stack_stride = static_cast<uint32_t>(threads); h->ref_stack_threads = threads;
  }
  AMBER_TRY(StartPixelMasks(h.get(), nullptr));   // asynchronous, on the render stream: in front of the handle's first launch
  h->build.create_ms = ms_since(t_create);
  *out = h.release();
  return AMBER_OK;
}

}  // namespace

extern "C" {

int amber_hip_abi_version(void) { return AMBER_HIP_ABI_VERSION; }
int amber_hip_math_mode(void) { return AMBER_MATH_MODE; }
int amber_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int amber_hip_pt_create(const AmberFlatScene* s, const AmberSensor* sensor, const AmberPtParams* params, amber_hip_pt** out) {
  return Guarded("amber_hip_pt_create", [&]() -> int {         // (std::system_error: std::async of the reference's build could not start a thread)
    if (!out || !params) return Fail(AMBER_EINVAL, "null argument");
    *out = nullptr;
    return Create(s, sensor, params, out);
  });
}

}  // extern "C"

namespace {
// Hands out the next event pair; when the pool of 64 is used up the finished launches are folded into the running
// totals (one stream synchronisation every 64 launches), so long renders (--spp 0 until expiry) do not grow the pool.
int AcquireEventPair(amber_hip_pt* h, std::pair<Event, Event>** out) {
  if (h->events_used == 64) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < h->events_used; i++) {
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, h->events[i].first.v, h->events[i].second.v));
      h->timed_ms += ms;
    }
    h->timed_launches += static_cast<uint32_t>(h->events_used);
    h->events_used = 0;
  }
  if (h->events_used == h->events.size()) {
    std::pair<Event, Event> ev;
    HIP_TRY(hipEventCreate(&ev.first.v)); HIP_TRY(hipEventCreate(&ev.second.v));
    h->events.push_back(std::move(ev));
  }
  *out = &h->events[h->events_used++];
  return AMBER_OK;
}

// Workgroups of the persistent kernels that fit a CU at once: pt_bvh_megakernel is bounded by its 24-entry LDS traversal stacks and
// VGPRs; the others are capped to AMBER_MEGAKERNEL_WAVES_PER_SIMD by their launch bounds.
uint32_t ResidentBlocksPerCu(uint32_t hit_engine) {
  return hit_engine == AMBER_ENGINE_BVH ? static_cast<uint32_t>(AMBER_BVH_WGS) : (AMBER_MEGAKERNEL_WAVES_PER_SIMD > 5 ? static_cast<uint32_t>(AMBER_MEGAKERNEL_WAVES_PER_SIMD) : 5u);   // uncapped: 87 VGPRs -> 5
}

// Workgroups of 256 threads for n_items work units (one thread each), `resident` at the most.
uint32_t BlocksFor(uint64_t n_items, uint32_t resident) {
  const uint64_t by_work = n_items / 256u + (n_items % 256u != 0u);
  return by_work < resident ? static_cast<uint32_t>(by_work) : resident;
}

// The grid of every persistent launch: workgroups of 256 threads, as many as fit the device at once, fewer if n_items work units (one
// thread each) do not need them.  The default n_items gives the largest grid, for which engine REFERENCE_BVH's stack is sized.  `pool`:
// pt_bvh_pool_kernel's grid (lab build).
uint32_t PersistentBlocks(const amber_hip_pt* h, uint64_t n_items, bool pool) {
  uint32_t n_blocks = static_cast<uint32_t>(h->n_cus) * ResidentBlocksPerCu(h->hit_engine);
#ifdef AMBER_LAB
  if (pool) n_blocks = static_cast<uint32_t>(h->n_cus) * static_cast<uint32_t>(AMBER_BVH_POOL_WGS);
#endif
  return BlocksFor(n_items, n_blocks);
}

// The one mapping from a handle's closest-hit engine to the engine its kernels are instantiated with: f(std::integral_constant<int, kEngine>).
// Each caller picks its kernel with `if constexpr`, so nothing is instantiated that is never launched.
template <typename F>
int WithHitEngine(uint32_t hit_engine, F&& f) {
  switch (hit_engine) {
    case AMBER_ENGINE_TWO_PHASE: return f(std::integral_constant<int, ENGINE_TWO_PHASE>());
    case kHitTwoPhaseN: return f(std::integral_constant<int, ENGINE_TWO_PHASE_N>());
    case AMBER_ENGINE_BVH: return f(std::integral_constant<int, ENGINE_BVH>());
    case AMBER_ENGINE_REFERENCE_BVH: return f(std::integral_constant<int, ENGINE_REF_BVH>());
    default: return f(std::integral_constant<int, ENGINE_LIST>());
  }
}

// Engine REFERENCE_BVH's stack has one column per thread of the largest grid (create; the handle remembers how many): a launch must not have more
// threads.  Every launch site of a kernel that walks that tree -- the render passes, light tracing, the ray queries, which share the one stack -- asks
// here first, before it takes anything (an event pair) it would have to give back.
int CheckRefStack(const amber_hip_pt* h, uint32_t n_blocks) {
  if (h->hit_engine == AMBER_ENGINE_REFERENCE_BVH && static_cast<uint64_t>(n_blocks) * 256u > h->ref_stack_threads)
    return Fail(AMBER_EINVAL, "engine REFERENCE_BVH: a grid of " + std::to_string(n_blocks) + " workgroups outgrows the traversal stack (" + std::to_string(h->ref_stack_threads) + " threads)");
  return AMBER_OK;
}

// Grows a buffer of the handle to at least n elements.  It may be in use: the stream is synchronised before it is freed.
template <typename T>
int Grow(amber_hip_pt* h, DevBuf<T>& b, size_t n, const char* what) {
  if (n <= b.n) return AMBER_OK;
  HIP_TRY(hipStreamSynchronize(h->stream));
  const hipError_t e = b.alloc(n);
  if (e != hipSuccess) return Fail(AMBER_ENOMEM, std::string("hipMalloc(") + what + "): " + hipGetErrorString(e));
  return AMBER_OK;
}

// What every launch of a render kernel states first: the scene, the seed, the handle's band, the samples and their chunks (with the dividers).
RenderArgs MakeRenderArgs(const amber_hip_pt* h, uint64_t hashed_seed, uint32_t n_pixels, uint32_t first_sample, uint32_t n_samples) {
  RenderArgs a{};
  a.scene = h->scene; a.hashed_seed = hashed_seed; a.SetBand(h->row_begin, h->stripe_rows, h->stripe_period); a.n_pixels = n_pixels;
  a.SetSamples(first_sample, n_samples); a.n_chunks = (n_samples + AMBER_ACCUM_CHUNK - 1) / AMBER_ACCUM_CHUNK;
  return a;
}

}  // namespace

namespace {
// ---- path-granular launches (pt_megakernel for engines LIST / TWO_PHASE, pt_bvh_pool_kernel for engine BVH) --------------
// One launch = megakernel + rank / scan / place / reduce.  The record buffer is sized from the density the previous launch
// measured (record slots per path), with a margin; the very first launch of a handle is one accumulation chunk, whose buffer
// can hold a record for EVERY path, and doubles as the probe.  A launch that still runs out of slots leaves the framebuffer
// and the ray total untouched (the device-side kernels check the counter); the host notices when it next touches the handle
// (ResolvePending), grows the buffer and repeats exactly that launch, so results never depend on the sizing.  Launches are
// split on chunk boundaries, which leaves the summation order unchanged.
constexpr uint64_t kMaxPathsPerLaunch = 1ull << 30;       // q and its bitmap index stay 32-bit; bitmap 128 MiB
constexpr uint64_t kMaxRecordSlots = 48ull << 20;         // 28 B per slot (record + sorted measurement): 1.3 GiB at most

// record slots that stay unused because every wave reserves them AMBER_REC_BLOCK at a time, plus a floor
uint64_t RecordSlack(const amber_hip_pt* h) { return static_cast<uint64_t>(h->n_cus) * 8u * 4u * AMBER_REC_BLOCK + 4096u; }

int EnsureRecordCapacity(amber_hip_pt* h, uint64_t slots) {
  if (slots <= h->rec_capacity) return AMBER_OK;
  if (slots > 0xfffffff0ull) return Fail(AMBER_ENOMEM, "record buffer beyond 2^32 slots");
  h->rec_capacity = 0;
  AMBER_TRY(Grow(h, h->d_records, slots, "path records"));
  AMBER_TRY(Grow(h, h->d_sorted, slots * 3u, "path records"));
  h->rec_capacity = static_cast<uint32_t>(slots);
  return AMBER_OK;
}

// Enqueues one launch over samples [first, first + n) of the band.  `sig` != nullptr: the signature variant of the same
// kernel; nothing is reduced (amber_hip_pt_signatures).
int EnsureLaunchCtl(amber_hip_pt* h) {                                       // queue head | record count | rays of the launch: one block, one memset per launch
  if (!h->d_launch_ctl) {
    HIP_TRY(h->d_launch_ctl.alloc(4));
    h->d_rec_count = h->d_launch_ctl + 1;
    h->d_rays_launch = reinterpret_cast<unsigned long long*>(h->d_launch_ctl + 2);
  }
  return AMBER_OK;
}

// Two-phase engine, once per handle: the candidate mask of every band pixel's eye rays (pixel_mask_kernel), enqueued on the render stream by
// create -- in front of the handle's first launch.  The buffer is allocated once and owned by the handle (amber_hip_pt_destroy releases it
// whatever step failed).  `timing` != null (amber_hip_kat_pixel_masks): run the kernel (again) between two events and report its duration.
int StartPixelMasks(amber_hip_pt* h, float* timing) {
  const uint32_t n_pixels = static_cast<uint32_t>(BandPixels(h));
  if (!(h->two_phase && h->env.pixel_mask) || n_pixels == 0 || (h->pixel_mask_ready && !timing)) return AMBER_OK;
  if (!h->d_pixel_mask) HIP_TRY(h->d_pixel_mask.alloc(n_pixels));
  PixelMaskArgs pm{};
  for (int i = 0; i < 4; i++) for (int c = 0; c < 3; c++) pm.ap[i][c] = static_cast<double>(h->aperture_rect[i][c]) - static_cast<double>(h->scene.fp_center[c]);
  pm.inv_w = 1.0 / static_cast<double>(h->scene.sensor.wf); pm.inv_h = 1.0 / static_cast<double>(h->scene.sensor.hf);
  pm.focal_scale = h->lens.kind == 1u ? -(8.0 * static_cast<double>(h->scene.fp_reach) + 1.0) / static_cast<double>(h->lens.sensor_distance)
                                      : static_cast<double>(h->lens.focus_distance) / -static_cast<double>(h->lens.sensor_distance);
  pm.row_begin = h->row_begin; pm.stripe_rows = h->stripe_rows; pm.stripe_period = h->stripe_period; pm.n_pixels = n_pixels;
  pm.block = (h->stripe_rows == 0u || h->stripe_rows % 4u == 0u) ? 4u : 1u;
  if (h->env.pixel_mask_block && (h->stripe_rows == 0u || h->stripe_rows % h->env.pixel_mask_block == 0u)) pm.block = h->env.pixel_mask_block;   // measurement hook
  pm.local_rows = h->local_rows;
  pm.blocks_x = (h->scene.sensor.w + pm.block - 1u) / pm.block;
  pm.n_blocks = pm.blocks_x * ((h->local_rows + pm.block - 1u) / pm.block);
  {
    // "does plane i cut the aperture rectangle?" -- the kernel's own expressions (binary64, the slack of its first lines), evaluated once
    const DevScene& sc = h->scene;
    const double cx = sc.fp_center[0], cy = sc.fp_center[1], cz = sc.fp_center[2], reach = sc.fp_reach;
    const double world_mag = std::max(std::max(std::fabs(cx), std::max(std::fabs(cy), std::fabs(cz))) + reach,
                                      std::max(std::fabs(double(h->lens.origin[0])), std::max(std::fabs(double(h->lens.origin[1])), std::fabs(double(h->lens.origin[2])))));
    const double slack = 1e-5 * reach + 32.0 * 5.9604644775390625e-08 * world_mag;
    pm.planes_cut_a = h->host_planes.size() > 32 ? 0xffffffffu : 0u;
    for (size_t i = 0; i < h->host_planes.size() && i < 32; i++) {
      const DevPlane& q = h->host_planes[i];
      bool above = true, below = true;
      for (int k = 0; k < 4; k++) {
        const double sa = double(q.n[0]) * pm.ap[k][0] + double(q.n[1]) * pm.ap[k][1] + double(q.n[2]) * pm.ap[k][2] - double(q.d0);
        above = above && sa > 10.0 * slack; below = below && sa < -10.0 * slack;
      }
      if (!(above || below)) pm.planes_cut_a |= 1u << i;
    }
  }
  Event ev0, ev1;
  if (timing) { HIP_TRY(hipEventCreate(&ev0.v)); HIP_TRY(hipEventCreate(&ev1.v)); HIP_TRY(hipEventRecord(ev0.v, h->stream)); }
  hipLaunchKernelGGL(pixel_mask_kernel, dim3((pm.n_blocks + 15u) / 16u), dim3(256), 0, h->stream, h->scene, pm, h->d_pixel_mask);   // 16 lanes per block of pixels
  HIP_TRY(hipGetLastError());
  if (timing) { HIP_TRY(hipEventRecord(ev1.v, h->stream)); HIP_TRY(hipEventSynchronize(ev1.v)); HIP_TRY(hipEventElapsedTime(timing, ev0.v, ev1.v)); }
  h->pixel_mask_ready = true;
  return AMBER_OK;
}

// pt_megakernel of the handle's engine, or pt_bvh_pool_kernel (`pool`, lab build); kSig: their signature instantiations
template <bool kSig>
void LaunchPathKernel(const amber_hip_pt* h, bool pool, uint32_t n_blocks, const RenderArgs& a) {
  WithHitEngine(h->hit_engine, [&](auto engine) -> int {
    constexpr int kEngine = decltype(engine)::value;
#ifdef AMBER_LAB
    if (kEngine == ENGINE_BVH && pool) { hipLaunchKernelGGL((pt_bvh_pool_kernel<kSig>), dim3(n_blocks), dim3(256), 0, h->stream, a); return AMBER_OK; }
#endif
    hipLaunchKernelGGL((pt_megakernel<kEngine, false, kSig>), dim3(n_blocks), dim3(256), 0, h->stream, a);
    return AMBER_OK;
  });
}

int LaunchPaths(amber_hip_pt* h, uint32_t first, uint32_t n, uint32_t n_pixels, unsigned long long* sig) {
  const uint64_t n_paths = static_cast<uint64_t>(n_pixels) * n;
#ifdef AMBER_LAB
  const bool bvh = h->hit_engine == AMBER_ENGINE_BVH && !h->bvh_paths;       // pt_bvh_pool_kernel (bvh_paths: pt_megakernel<ENGINE_BVH>)
#else
  const bool bvh = false;
  if (sig) return Fail(AMBER_EINVAL, "path signatures are part of the lab build");
#endif
  const size_t need_words = static_cast<size_t>((n_paths + 31u) / 32u) + 4u;
  if (need_words > h->d_flags.n) {
    AMBER_TRY(Grow(h, h->d_flags, need_words, "path bitmap"));
    h->flags_dirty = true;
  }
  const size_t touched_words = static_cast<size_t>(n_pixels) / 32u + 2u;
  AMBER_TRY(Grow(h, h->d_touched, touched_words, "touched pixels"));
  AMBER_TRY(Grow(h, h->d_excl, n_pixels, "pixel ranks"));
  AMBER_TRY(Grow(h, h->d_block_sum, static_cast<size_t>(n_pixels) / 256u + 2u, "pixel ranks"));
  AMBER_TRY(EnsureLaunchCtl(h));
  if (!h->h_rec_count.v) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->h_rec_count.v), sizeof(unsigned int), hipHostMallocDefault));
  if (!h->pending_event.v) HIP_TRY(hipEventCreateWithFlags(&h->pending_event.v, hipEventDisableTiming));
  const uint32_t n_blocks = PersistentBlocks(h, n_paths, bvh);
  AMBER_TRY(CheckRefStack(h, n_blocks));
  {
    // measurements carried across bounces (degenerate paths only): pt_megakernel 3 floats per thread of the grid, pt_bvh_pool_kernel per ray of a wave
    size_t carried = static_cast<size_t>(PersistentBlocks(h)) * 256u * 3u * 2u;   // own slots + parked slots
#ifdef AMBER_LAB
    if (bvh) carried = static_cast<size_t>(h->n_cus) * AMBER_BVH_POOL_WGS * 4u * AMBER_BVH_POOL_CARRIED_PER_WAVE;
#endif
    AMBER_TRY(Grow(h, h->d_carried, carried, "carried measurements"));
  }
#ifdef AMBER_LAB
  if (bvh) AMBER_TRY(Grow(h, h->d_bvh_stack, static_cast<size_t>(h->n_cus) * AMBER_BVH_POOL_WGS * 256u * AMBER_BVH_POOL_GLOBAL_LEVELS, "traversal stacks"));
#endif
  RenderArgs a = MakeRenderArgs(h, h->hashed_seed, n_pixels, first, n);
  a.pixel_mask = h->pixel_mask_ready ? h->d_pixel_mask : nullptr;
  a.flags = h->d_flags; a.touched = h->d_touched; a.records = h->d_records; a.rec_count = h->d_rec_count; a.rec_capacity = h->rec_capacity;
  a.ray_count = h->d_rays_launch; a.next_item = h->d_launch_ctl; a.stamps = h->d_stamps;
  a.bvh_stack = h->d_bvh_stack; a.carried = h->d_carried; a.sig = sig; a.n_items = static_cast<uint32_t>(n_paths);
  HIP_TRY(hipMemsetAsync(h->d_launch_ctl, 0, 4 * sizeof(unsigned int), h->stream));
  // The bitmap is cleared by the reduction itself where it can be (whole words per pixel); the host clears all of it only when a
  // launch left it dirty: the first use, sample counts that are not multiples of 32, signature launches, a launch that ran out of slots.
  if (h->flags_dirty) HIP_TRY(hipMemsetAsync(h->d_flags, 0, h->d_flags.n * sizeof(uint32_t), h->stream));
  h->flags_dirty = sig != nullptr || (n & 31u) != 0u;
  HIP_TRY(hipMemsetAsync(h->d_touched, 0, touched_words * sizeof(uint32_t), h->stream));
  std::pair<Event, Event>* evp = nullptr;
  AMBER_TRY(AcquireEventPair(h, &evp));
  auto& ev = *evp;
  HIP_TRY(hipEventRecord(ev.first.v, h->stream));
#ifdef AMBER_LAB
  if (sig) LaunchPathKernel<true>(h, bvh, n_blocks, a);      // the signature instantiations of the same kernels (amber_hip_pt_signatures)
  else
#endif
  LaunchPathKernel<false>(h, bvh, n_blocks, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ev.second.v, h->stream));
  if (sig) return AMBER_OK;
  const uint32_t n_rank_blocks = (n_pixels + 255u) / 256u;
  hipLaunchKernelGGL(rec_rank_kernel, dim3(n_rank_blocks), dim3(256), 0, h->stream, h->d_flags, h->d_touched, n_pixels, n, h->d_excl, h->d_block_sum);
  hipLaunchKernelGGL(rec_scan_blocks_kernel, dim3(1), dim3(1024), 0, h->stream, h->d_block_sum, n_rank_blocks, h->d_rec_count, h->rec_capacity, h->d_rays, h->d_rays_launch);
  hipLaunchKernelGGL(rec_place_kernel, dim3(static_cast<uint32_t>(h->n_cus) * 8u), dim3(256), 0, h->stream, h->d_records, h->d_rec_count, h->rec_capacity, h->d_flags,
                     h->d_excl, h->d_block_sum, n, MakeExactDiv(n), h->d_sorted);
  hipLaunchKernelGGL(reduce_flagged_kernel, dim3(n_rank_blocks), dim3(256), 0, h->stream, h->accum_target, h->d_flags, h->d_touched, h->d_sorted, h->d_excl, h->d_block_sum,
                     h->d_rec_count, h->rec_capacity, n_pixels, n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h->h_rec_count.v, h->d_rec_count, sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipEventRecord(h->pending_event.v, h->stream));
  h->pending = true; h->pending_first = first; h->pending_n = n; h->pending_target = h->accum_target;
  h->pending_checked = n_paths + RecordSlack(h) <= h->rec_capacity;      // a slot for every path: cannot run out
  return AMBER_OK;
}

// Looks at the record counter of the launch in flight (waits for it), remembers the density, and repeats the launch with a
// larger buffer if it ran out of slots.  Every entry point that reads results, or enqueues work whose order matters, calls it.
int ResolvePending(amber_hip_pt* h) {
  while (h->pending) {
    HIP_TRY(hipEventSynchronize(h->pending_event.v));
    h->pending = false;
    const uint64_t used = *h->h_rec_count.v;
    const uint64_t n_paths = BandPixels(h) * h->pending_n;
    h->rec_density = n_paths ? static_cast<double>(used) / static_cast<double>(n_paths) : 0.0;
    h->density_known = true;
    if (used <= h->rec_capacity) break;
    // out of slots: nothing of that launch reached the framebuffer or the ray total (and its bits are still set)
    h->flags_dirty = true;
    AMBER_TRY(EnsureRecordCapacity(h, used + used / 4u + RecordSlack(h)));
    float* const target = h->accum_target;
    h->accum_target = h->pending_target;
    const int rl = LaunchPaths(h, h->pending_first, h->pending_n, static_cast<uint32_t>(BandPixels(h)), nullptr);
    h->accum_target = target;
    if (rl != AMBER_OK) return rl;
  }
  return AMBER_OK;
}

int RenderPassPaths(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples, uint32_t n_pixels) {
  uint64_t max_samples = kMaxPathsPerLaunch / n_pixels / AMBER_ACCUM_CHUNK * AMBER_ACCUM_CHUNK;
  if (max_samples == 0) return Fail(AMBER_EINVAL, "band too large for one launch");
  const uint64_t slack = h->env.test_density_scale > 0 ? 64u : RecordSlack(h);   // (test hook: no cushion either)
  uint32_t done = 0;
  while (done < n_samples) {
    // the previous launch must stand before the next one adds to the framebuffer (the order of the sums is part of the
    // contract), unless it had a slot for every path
    if (h->pending && (!h->pending_checked || !h->density_known)) AMBER_TRY(ResolvePending(h));
    uint32_t n = n_samples - done;
    if (n > max_samples) n = static_cast<uint32_t>(max_samples);
    uint64_t slots;
    if (!h->density_known) {
      // first launch of the handle: a slot for every path, and at most one chunk unless the job is small -- it measures the density
      if (static_cast<uint64_t>(n_pixels) * n > (4ull << 20) && n > AMBER_ACCUM_CHUNK) n = AMBER_ACCUM_CHUNK;
      slots = static_cast<uint64_t>(n_pixels) * n + slack;
    } else {
      double density = h->rec_density;
      if (h->env.test_density_scale > 0) density *= h->env.test_density_scale;   // test hook: a wrong estimate must only cost a repeated launch
      const double per_sample = std::max(1e-9, density * 1.5) * static_cast<double>(n_pixels);   // slots one sample of the band needs, with margin
      const uint64_t all = static_cast<uint64_t>(n_pixels) * n;
      const double want = per_sample * n;
      if (want + static_cast<double>(slack) > static_cast<double>(kMaxRecordSlots) && all + slack > kMaxRecordSlots) {
        // a dense scene: shorter launches instead of a larger buffer
        uint64_t fit = static_cast<uint64_t>((static_cast<double>(kMaxRecordSlots) - static_cast<double>(slack)) / per_sample) / AMBER_ACCUM_CHUNK * AMBER_ACCUM_CHUNK;
        if (fit < AMBER_ACCUM_CHUNK) fit = AMBER_ACCUM_CHUNK;
        if (n > fit) n = static_cast<uint32_t>(fit);
      }
      const uint64_t all_n = static_cast<uint64_t>(n_pixels) * n;
      slots = std::min<uint64_t>(all_n, static_cast<uint64_t>(per_sample * n) + 1u) + slack;
    }
    if (slots > h->rec_capacity) {
      if (h->pending) AMBER_TRY(ResolvePending(h));     // the buffer is in use
      AMBER_TRY(EnsureRecordCapacity(h, slots));
    }
    AMBER_TRY(LaunchPaths(h, first_sample + done, n, n_pixels, nullptr));
    done += n;
  }
  return AMBER_OK;
}

// The launches of light tracing over the passes [first_sample, first_sample + n_samples) of the light paths [path_begin, path_begin + n_paths): what
// amber_hip_lt_trace_range and amber_hip_lt_render_pass share.  Each launch leaves its splat records at h->d_splats in arrival order (at most
// `capacity` of them, read again before every launch: the callback may have grown the buffer) and is waited for; then
//   after_launch(first, n, produced, rays_before, rays_now, &again)
// sees the passes of the launch, the records it produced (also beyond the capacity) and the handle's ray counter before the first launch and now.
// It returns a status other than AMBER_OK to stop, or sets `again` to have exactly this launch repeated.  `timed`: amber_hip_pt_kernel_time counts
// the launches.  n_samples and n_paths are not zero.
template <typename F>
int LtTraceLaunches(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples, uint32_t path_begin, uint32_t n_paths, bool timed, const uint32_t& capacity, F&& after_launch) {
  const bool bvh = h->hit_engine == AMBER_ENGINE_BVH;
  // One launch numbers its work units with 31 bits -- pt_megakernel: (light path, pass) pairs; pt_bvh_megakernel: (light
  // path, chunk of passes) items -- so a long range of passes is traced in several launches, each a whole number of chunks.
  // Launches run in pass order and each one's splats are sorted, so the concatenation is in (pass, path, bounce) order.
  const uint64_t max_units = 0x7fffffffull / n_paths;
  if (max_units == 0) return Fail(AMBER_EINVAL, "too many light paths for one launch");
  uint64_t max_samples = bvh ? max_units * AMBER_ACCUM_CHUNK : max_units / AMBER_ACCUM_CHUNK * AMBER_ACCUM_CHUNK;
  if (max_samples == 0) max_samples = max_units;               // fewer than a chunk fits: any split is valid for light tracing (nothing is summed across launches)
  unsigned long long rays_before = 0, rays_now = 0;
  HIP_TRY(hipMemcpyAsync(&rays_before, h->d_rays, sizeof rays_before, hipMemcpyDeviceToHost, h->stream));
  uint32_t done = 0;
  while (done < n_samples) {
    uint32_t n = n_samples - done;
    if (n > max_samples) n = static_cast<uint32_t>(max_samples);
    const uint32_t n_chunks = (n + AMBER_ACCUM_CHUNK - 1) / AMBER_ACCUM_CHUNK;
    const uint64_t n_work = bvh ? static_cast<uint64_t>(n_paths) * n_chunks : static_cast<uint64_t>(n_paths) * n;
    RenderArgs a = MakeRenderArgs(h, h->hashed_seed_lt, n_paths, first_sample + done, n);
    a.SetBand(0u, 0u, 0u);                                    // light paths have no band; every divider of the launch is a valid record all the same
    a.ray_count = h->d_rays; a.next_item = h->d_next;
    a.splats = h->d_splats; a.splat_count = h->d_splat_count; a.splat_capacity = capacity;
    a.path_offset = path_begin; a.n_items = static_cast<uint32_t>(n_work); a.shade_batch = h->bvh_shade_batch;
    const uint32_t n_blocks = PersistentBlocks(h, a.n_items);
    AMBER_TRY(CheckRefStack(h, n_blocks));
    std::pair<Event, Event>* evp = nullptr;
    if (timed) AMBER_TRY(AcquireEventPair(h, &evp));
    HIP_TRY(hipMemsetAsync(h->d_splat_count, 0, sizeof(unsigned int), h->stream));
    HIP_TRY(hipMemsetAsync(h->d_next, 0, sizeof(unsigned int), h->stream));
    if (evp) HIP_TRY(hipEventRecord(evp->first.v, h->stream));
    WithHitEngine(h->hit_engine, [&](auto engine) -> int {
      constexpr int kEngine = decltype(engine)::value;
      if constexpr (kEngine == ENGINE_BVH) hipLaunchKernelGGL((pt_bvh_megakernel<true, 24>), dim3(n_blocks), dim3(256), 0, h->stream, a);   // light tracing on engine BVH: always the item kernel
      else hipLaunchKernelGGL((pt_megakernel<kEngine, true>), dim3(n_blocks), dim3(256), 0, h->stream, a);
      return AMBER_OK;
    });
    HIP_TRY(hipGetLastError());
    if (evp) HIP_TRY(hipEventRecord(evp->second.v, h->stream));
    unsigned int produced = 0;
    HIP_TRY(hipMemcpyAsync(&produced, h->d_splat_count, sizeof produced, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&rays_now, h->d_rays, sizeof rays_now, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    bool again = false;
    AMBER_TRY(after_launch(first_sample + done, n, produced, rays_before, rays_now, &again));
    if (!again) done += n;
  }
  return AMBER_OK;
}
}  // namespace

#include "ray_query.inc"
#include "image_stage.inc"
#include "resolve.inc"
#include "aov.inc"
#include "denoise.inc"
#include "denoise_variance.inc"
#include "temporal.inc"
#include "lt_accumulate.inc"

extern "C" {

static int RenderPassBvhItems(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples, uint32_t n_pixels, unsigned long long* sig);   // internal: not part of the ABI
#ifdef AMBER_LAB
namespace { int RenderPassWavefront(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples); }      // lab_api.inc
#endif

int amber_hip_pt_render_pass(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples) { return Guarded("amber_hip_pt_render_pass", [&]() -> int {
  if (!h) return Fail(AMBER_EINVAL, "null handle");
  if (n_samples == 0) return AMBER_OK;
  if (static_cast<uint64_t>(first_sample) + n_samples > 0xffffffffull) return Fail(AMBER_EINVAL, "sample index overflow");
  HIP_TRY(hipSetDevice(h->device));
  const uint32_t n_pixels = static_cast<uint32_t>(BandPixels(h));
  if (n_pixels == 0) return AMBER_OK;                    // empty band
#ifdef AMBER_LAB
  if (h->engine == AMBER_ENGINE_WAVEFRONT) return RenderPassWavefront(h, first_sample, n_samples);
#endif
  if (h->hit_engine != AMBER_ENGINE_BVH || h->bvh_pool || h->bvh_paths) return RenderPassPaths(h, first_sample, n_samples, n_pixels);
  return RenderPassBvhItems(h, first_sample, n_samples, n_pixels, nullptr);
}); }

// render_pass into the handle's batch buffer (zeroed) instead of the framebuffer, then moments_fold_kernel: fb = fb + B and the batch's luminance into
// the moments.  The accumulation target points at the batch buffer only inside this call: every way out restores it.
int amber_hip_pt_render_batch(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples) { return Guarded("amber_hip_pt_render_batch", [&]() -> int {
  const std::string name = "amber_hip_pt_render_batch";
  if (!h) return Fail(AMBER_EINVAL, name + ": null handle");
  if (n_samples == 0) return AMBER_OK;
  if (static_cast<uint64_t>(first_sample) + n_samples > 0xffffffffull) return Fail(AMBER_EINVAL, name + ": sample index overflow");
  HIP_TRY(hipSetDevice(h->device));
  const uint32_t n_pixels = static_cast<uint32_t>(BandPixels(h));
  if (n_pixels == 0) return AMBER_OK;                    // empty band
  if (h->engine == AMBER_ENGINE_WAVEFRONT) return Fail(AMBER_EINVAL, name + ": not part of the lab engine WAVEFRONT");
  // a pass in flight whose record buffer was sized from an estimate may have to be repeated: it must stand before the target moves
  if (h->pending && !h->pending_checked) AMBER_TRY(ResolvePending(h));
  AMBER_TRY(EnsureMoments(h, name.c_str()));
  AMBER_TRY(Grow(h, h->img.batch, static_cast<size_t>(n_pixels) * 3u, "batch sums"));
  HIP_TRY(hipMemsetAsync(h->img.batch, 0, static_cast<size_t>(n_pixels) * 3u * sizeof(float), h->stream));
  {
    struct Target {
      amber_hip_pt* h;
      explicit Target(amber_hip_pt* handle) : h(handle) { h->accum_target = h->img.batch; }
      ~Target() { h->accum_target = h->d_fb; }
    } target(h);
    int rc = (h->hit_engine != AMBER_ENGINE_BVH || h->bvh_pool || h->bvh_paths) ? RenderPassPaths(h, first_sample, n_samples, n_pixels)
                                                                                 : RenderPassBvhItems(h, first_sample, n_samples, n_pixels, nullptr);
    // ... and so must the batch's own last launch before the fold reads its sums (as amber_hip_pt_resolve waits)
    if (rc == AMBER_OK && h->pending && !h->pending_checked) rc = ResolvePending(h);
    // (after a failure here a launch may stay pending with the batch buffer for its target: a repeat of it then adds to a buffer nobody reads -- the
    // next batch zeroes it behind that repeat on the stream -- so nothing of a failed batch reaches the framebuffer or the moments)
    if (rc != AMBER_OK) return rc;
  }
  return FoldBatch(h, n_samples);
}); }

// sig != null (amber_hip_pt_signatures): one launch of the signature instantiation; nothing reaches the framebuffer or the ray total
static int RenderPassBvhItems(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples, uint32_t n_pixels, unsigned long long* sig) {
  // engine BVH, default scheduler (pt_bvh_megakernel: lanes own (pixel, chunk) items).  A launch covers at most kMaxPartialFloats
  // of per-item sums and < 2^31 items; longer passes are split on chunk boundaries, which leaves the summation order unchanged
#ifndef AMBER_LAB
  if (sig) return Fail(AMBER_EINVAL, "path signatures are part of the lab build");
#endif
  const uint64_t kMaxPartialFloats = 768ull << 20;    // 3 GiB
  uint64_t max_chunks = kMaxPartialFloats / (static_cast<uint64_t>(n_pixels) * 3u);
  const uint64_t by_items = 0x7fffffffull / n_pixels;
  if (by_items < max_chunks) max_chunks = by_items;
  if (max_chunks == 0) return Fail(AMBER_EINVAL, "band too large for one launch");
  uint32_t done = 0;
  while (done < n_samples) {
    uint32_t n = n_samples - done;
    const uint64_t cap = max_chunks * AMBER_ACCUM_CHUNK;
    if (n > cap) n = static_cast<uint32_t>(cap);
    const uint32_t n_chunks = (n + AMBER_ACCUM_CHUNK - 1) / AMBER_ACCUM_CHUNK;
    const size_t need = static_cast<size_t>(n_chunks) * n_pixels * 3u;
    AMBER_TRY(Grow(h, h->d_partial, need, "partial sums"));
    if (sig && n != n_samples) return Fail(AMBER_EINVAL, "too many paths for one signature launch");
    if (sig) AMBER_TRY(EnsureLaunchCtl(h));
    RenderArgs a = MakeRenderArgs(h, h->hashed_seed, n_pixels, first_sample + done, n);
    a.partial = h->d_partial; a.ray_count = sig ? h->d_rays_launch : h->d_rays; a.next_item = h->d_next; a.stamps = h->d_stamps;
    a.n_items = n_pixels * n_chunks; a.sig = sig; a.shade_batch = h->bvh_shade_batch;
    // persistent workers: one workgroup of 4 waves per CU and resident wave slot, fewer if the queue is short
    const uint32_t n_blocks = PersistentBlocks(h, a.n_items);
    HIP_TRY(hipMemsetAsync(h->d_next, 0, sizeof(unsigned int), h->stream));
    std::pair<Event, Event>* evp = nullptr;
    AMBER_TRY(AcquireEventPair(h, &evp));
    auto& ev = *evp;
    HIP_TRY(hipEventRecord(ev.first.v, h->stream));
#ifdef AMBER_LAB
    if (sig) hipLaunchKernelGGL((pt_bvh_megakernel<false, 24, true>), dim3(n_blocks), dim3(256), 0, h->stream, a);
    else
#endif
    hipLaunchKernelGGL((pt_bvh_megakernel<false, 24>), dim3(n_blocks), dim3(256), 0, h->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.second.v, h->stream));
    if (sig) return AMBER_OK;                                  // the signature launch: nothing reaches the framebuffer
    const uint32_t n_elems = n_pixels * 3u;
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((n_elems + 255u) / 256u), dim3(256), 0, h->stream, h->accum_target, h->d_partial, n_elems, n_chunks);
    HIP_TRY(hipGetLastError());
    done += n;
  }
  return AMBER_OK;
}

int amber_hip_lt_trace_range(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples, uint32_t path_begin, uint32_t path_end,
                             AmberSplat* out, uint32_t capacity, uint32_t* n_out, uint64_t* ray_count) { return Guarded("amber_hip_lt_trace_range", [&]() -> int {
  if (!h || !n_out || (capacity && !out)) return Fail(AMBER_EINVAL, "null argument");
  *n_out = 0;
  if (ray_count) *ray_count = 0;
  if (h->engine == AMBER_ENGINE_WAVEFRONT) return Fail(AMBER_EINVAL, "light tracing runs on the work-queue kernel (engine auto, list, two_phase or bvh)");
  if (h->lights_stale) return Fail(AMBER_EINVAL, "lights are stale after amber_hip_pt_update_objects: re-create the handle");
  if (static_cast<uint64_t>(first_sample) + n_samples > 0xffffffffull) return Fail(AMBER_EINVAL, "sample index overflow");
  const uint32_t all_paths = h->scene.sensor.w * h->scene.sensor.h;          // image.Size() light paths per pass
  if (path_begin > path_end || path_end > all_paths) return Fail(AMBER_EINVAL, "bad light-path range");
  const uint32_t n_paths = path_end - path_begin;
  if (n_samples == 0 || n_paths == 0 || h->scene.n_lights == 0) return AMBER_OK;
  HIP_TRY(hipSetDevice(h->device));
  AMBER_TRY(ResolvePending(h));
  const uint32_t dev_capacity = capacity ? capacity : 1u;
  AMBER_TRY(Grow(h, h->d_splats, dev_capacity, "splats"));
  if (!h->d_splat_count) HIP_TRY(h->d_splat_count.alloc(1));
  uint64_t total = 0;                                         // splats produced (also beyond the caller's capacity)
  unsigned long long rays_first = 0, rays_last = 0;
  bool any = false;
  const int rc = LtTraceLaunches(h, first_sample, n_samples, path_begin, n_paths, false, dev_capacity,
                                 [&](uint32_t, uint32_t, unsigned int produced, unsigned long long rays_before, unsigned long long rays_now, bool*) -> int {
    if (!any) { rays_first = rays_before; any = true; }
    rays_last = rays_now;
    const uint64_t room = total < capacity ? capacity - total : 0;
    if (produced <= room && produced <= dev_capacity) {
      if (produced) {
        static_assert(sizeof(AmberSplat) == sizeof(DevSplat), "splat layouts must agree");
        AmberSplat* dst = out + total;
        HIP_TRY(hipMemcpy(dst, h->d_splats, static_cast<size_t>(produced) * sizeof(DevSplat), hipMemcpyDeviceToHost));
        // the reference adds the splats of pass s in path order (algorithm_lt.cc:112-123): restore that order
        std::sort(dst, dst + produced, [](const AmberSplat& x, const AmberSplat& y) {
          if (x.sample != y.sample) return x.sample < y.sample;
          if (x.path != y.path) return x.path < y.path;
          return x.bounce < y.bounce;
        });
      }
    }
    total += produced;                                        // keeps counting: the caller learns the capacity it needs
    return AMBER_OK;
  });
  if (rc != AMBER_OK) return rc;
  if (ray_count) *ray_count = rays_last - rays_first;
  *n_out = total > 0xffffffffull ? 0xffffffffu : static_cast<uint32_t>(total);
  if (total > capacity) return Fail(AMBER_ENOMEM, "splat buffer too small: " + std::to_string(total) + " splats produced");
  return AMBER_OK;
}); }

int amber_hip_lt_render_pass(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples, AmberLtPassInfo* info) {
  return Guarded("amber_hip_lt_render_pass", [&] { return LtRenderPass(h, first_sample, n_samples, info); });
}

int amber_hip_lt_trace(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples, AmberSplat* out, uint32_t capacity,
                       uint32_t* n_out, uint64_t* ray_count) {
  return Guarded("amber_hip_lt_trace", [&]() -> int {
    return h ? amber_hip_lt_trace_range(h, first_sample, n_samples, 0u, h->scene.sensor.w * h->scene.sensor.h, out, capacity, n_out, ray_count) : Fail(AMBER_EINVAL, "null argument");
  });
}

int amber_hip_pt_clear(amber_hip_pt* h) { return Guarded("amber_hip_pt_clear", [&]() -> int {
  if (!h) return Fail(AMBER_EINVAL, "null handle");
  HIP_TRY(hipSetDevice(h->device));
  AMBER_TRY(ResolvePending(h));
  const size_t fb_floats = static_cast<size_t>(BandPixels(h)) * 3u;
  HIP_TRY(hipMemsetAsync(h->d_fb, 0, fb_floats * sizeof(float), h->stream));
  HIP_TRY(hipMemsetAsync(h->d_rays, 0, sizeof(unsigned long long), h->stream));
  // (no host synchronisation: the two fills are ordered on the handle's stream like everything else; event pairs handed out before
  //  this call have either been read by kernel_time() or are dropped here)
  h->events_used = 0; h->timed_launches = 0; h->timed_ms = 0;
  return AMBER_OK;
}); }

int amber_hip_pt_sync(amber_hip_pt* h) { return Guarded("amber_hip_pt_sync", [&]() -> int {
  if (!h) return Fail(AMBER_EINVAL, "null handle");
  HIP_TRY(hipSetDevice(h->device));
  AMBER_TRY(ResolvePending(h));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return AMBER_OK;
}); }

int amber_hip_pt_download(amber_hip_pt* h, float* rgb_sum, uint64_t* ray_count) { return Guarded("amber_hip_pt_download", [&]() -> int {
  if (!h) return Fail(AMBER_EINVAL, "null handle");
  HIP_TRY(hipSetDevice(h->device));
  AMBER_TRY(ResolvePending(h));
  const size_t fb_floats = static_cast<size_t>(BandPixels(h)) * 3u;
  if (rgb_sum) HIP_TRY(hipMemcpyAsync(rgb_sum, h->d_fb, fb_floats * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  unsigned long long r = 0;
  HIP_TRY(hipMemcpyAsync(&r, h->d_rays, sizeof r, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (ray_count) *ray_count = r;
  return AMBER_OK;
}); }

int amber_hip_pt_device_framebuffer(amber_hip_pt* h, void** dptr, uint64_t* n_floats) { return Guarded("amber_hip_pt_device_framebuffer", [&]() -> int {
  if (!h || !dptr) return Fail(AMBER_EINVAL, "null argument");
  *dptr = h->d_fb;
  if (n_floats) *n_floats = BandPixels(h) * 3;
  return AMBER_OK;
}); }

int amber_hip_pt_stream(amber_hip_pt* h, void** stream) { return Guarded("amber_hip_pt_stream", [&]() -> int {
  if (!h || !stream) return Fail(AMBER_EINVAL, "null argument");
  *stream = h->stream;
  return AMBER_OK;
}); }

int amber_hip_pt_local_rows(amber_hip_pt* h, uint32_t* n_rows) { return Guarded("amber_hip_pt_local_rows", [&]() -> int {
  if (!h || !n_rows) return Fail(AMBER_EINVAL, "null argument");
  *n_rows = h->local_rows;
  return AMBER_OK;
}); }

int amber_hip_pt_update_objects(amber_hip_pt* h, uint32_t first, uint32_t count, const AmberFlatObject* objects, uint32_t mode, AmberUpdateInfo* info) {
  return Guarded("amber_hip_pt_update_objects", [&]() -> int { return h ? UpdateObjects(h, first, count, objects, mode, info) : Fail(AMBER_EINVAL, "null handle"); });
}

int amber_hip_pt_update_lens(amber_hip_pt* h, const AmberFlatThinLens* lens, const AmberFlatObject* blades, uint32_t mode, AmberUpdateInfo* info) {
  return Guarded("amber_hip_pt_update_lens", [&]() -> int { return h ? UpdateLens(h, lens, blades, mode, info) : Fail(AMBER_EINVAL, "null handle"); });
}

int amber_hip_pt_cast_rays(amber_hip_pt* h, uint64_t n, const AmberRay* rays, AmberRayHit* hits, uint32_t flags) {
  return Guarded("amber_hip_pt_cast_rays", [&] { return RayQuery(h, n, rays, hits, flags, false, "amber_hip_pt_cast_rays"); });
}

int amber_hip_pt_occluded(amber_hip_pt* h, uint64_t n, const AmberRay* rays, uint8_t* occluded, uint32_t flags) {
  return Guarded("amber_hip_pt_occluded", [&] { return RayQuery(h, n, rays, occluded, flags, true, "amber_hip_pt_occluded"); });
}

int amber_hip_pt_resolve(amber_hip_pt* h, uint32_t n_samples, uint32_t format, void* out, uint64_t out_bytes, uint32_t flags) {
  return Guarded("amber_hip_pt_resolve", [&] { return Resolve(h, n_samples, format, out, out_bytes, flags); });
}

int amber_hip_pt_aov_pass(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples) {
  return Guarded("amber_hip_pt_aov_pass", [&] { return AovPass(h, first_sample, n_samples); });
}

int amber_hip_pt_aov_clear(amber_hip_pt* h) {
  return Guarded("amber_hip_pt_aov_clear", [&] { return AovClear(h); });
}

int amber_hip_pt_aov_download(amber_hip_pt* h, AmberAovPixel* out) {
  return Guarded("amber_hip_pt_aov_download", [&] { return AovDownload(h, out); });
}

int amber_hip_pt_device_aov(amber_hip_pt* h, void** dptr, uint64_t* n_pixels) {
  return Guarded("amber_hip_pt_device_aov", [&] { return DeviceAov(h, dptr, n_pixels); });
}

int amber_hip_pt_denoise(amber_hip_pt* h, uint32_t n_samples, const AmberDenoiseParams* params, uint32_t format, void* out, uint64_t out_bytes, uint32_t flags) {
  return Guarded("amber_hip_pt_denoise", [&] { return Denoise(h, n_samples, params, format, out, out_bytes, flags); });
}

int amber_hip_pt_temporal(amber_hip_pt* h, uint32_t n_samples, const AmberTemporalParams* params, uint32_t format, void* out, uint64_t out_bytes, uint32_t flags) {
  return Guarded("amber_hip_pt_temporal", [&] { return Temporal(h, n_samples, params, format, out, out_bytes, flags); });
}

int amber_hip_pt_temporal_reset(amber_hip_pt* h) {
  return Guarded("amber_hip_pt_temporal_reset", [&] { return TemporalReset(h); });
}

int amber_hip_pt_history_download(amber_hip_pt* h, AmberHistoryPixel* out) {
  return Guarded("amber_hip_pt_history_download", [&] { return HistoryDownload(h, out); });
}

int amber_hip_pt_device_history(amber_hip_pt* h, void** dptr, uint64_t* n_pixels) {
  return Guarded("amber_hip_pt_device_history", [&] { return DeviceHistory(h, dptr, n_pixels); });
}

int amber_hip_pt_moments_clear(amber_hip_pt* h) {
  return Guarded("amber_hip_pt_moments_clear", [&] { return MomentsClear(h); });
}

int amber_hip_pt_moments_download(amber_hip_pt* h, AmberMomentsPixel* out) {
  return Guarded("amber_hip_pt_moments_download", [&] { return MomentsDownload(h, out); });
}

int amber_hip_pt_device_moments(amber_hip_pt* h, void** dptr, uint64_t* n_pixels) {
  return Guarded("amber_hip_pt_device_moments", [&] { return DeviceMoments(h, dptr, n_pixels); });
}

int amber_hip_pt_denoise_variance(amber_hip_pt* h, uint32_t n_samples, const AmberDenoiseVarianceParams* params, uint32_t format, void* out, uint64_t out_bytes, uint32_t flags) {
  return Guarded("amber_hip_pt_denoise_variance", [&] { return DenoiseVariance(h, n_samples, params, format, out, out_bytes, flags); });
}

int amber_hip_pt_build_info(amber_hip_pt* h, AmberBuildInfo* out) { return Guarded("amber_hip_pt_build_info", [&]() -> int {
  if (!h || !out) return Fail(AMBER_EINVAL, "null argument");
  *out = h->build;
  return AMBER_OK;
}); }

int amber_hip_pt_kernel_time(amber_hip_pt* h, uint32_t* n_launches, double* total_ms) { return Guarded("amber_hip_pt_kernel_time", [&]() -> int {
  if (!h) return Fail(AMBER_EINVAL, "null handle");
  HIP_TRY(hipSetDevice(h->device));
  AMBER_TRY(ResolvePending(h));
  HIP_TRY(hipStreamSynchronize(h->stream));
  double tot = h->timed_ms;
  for (size_t i = 0; i < h->events_used; i++) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->events[i].first.v, h->events[i].second.v));
    tot += ms;
  }
  if (n_launches) *n_launches = h->timed_launches + static_cast<uint32_t>(h->events_used);
  if (total_ms) *total_ms = tot;
  return AMBER_OK;
}); }

#ifdef AMBER_STAMPS
// diagnostic build only: per wave of the last pt_megakernel launch, wall-clock ticks (100 MHz) at start, after the first claim,
// when it found the queue empty, at its end (tools/wave_times.py)
extern "C" int amber_hip_pt_read_wave_times(amber_hip_pt* h, unsigned long long* out, unsigned int n_waves) {
  if (!h || !h->d_stamps || n_waves > AMBER_WAVE_TIME_SLOTS) return AMBER_EINVAL;
  (void)hipStreamSynchronize(h->stream);
  return hipMemcpy(out, h->d_stamps + 8, 4ull * n_waves * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess ? AMBER_OK : AMBER_EHIP;
}
extern "C" int amber_hip_pt_read_stamps(amber_hip_pt* h, unsigned long long out[8]) {
  if (!h || !h->d_stamps) return AMBER_EINVAL;
  (void)hipStreamSynchronize(h->stream);
  return hipMemcpy(out, h->d_stamps, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess ? AMBER_OK : AMBER_EHIP;
}
#endif

void amber_hip_pt_destroy(amber_hip_pt* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;            // the owners release every buffer, event and pinned counter, then the handle's own stream
}

}  // extern "C"

#ifdef AMBER_LAB
#include "lab_api.inc"
#endif

// pt_host.hip -- the ONE translation unit of the gfx950 path-tracing engine: the handle, create and the C ABI (include/amber_hip.h).  The kernels and
// the host side of their launches live in files of their own and are included here:
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
//   launch_plan.h, pt_launch.inc   the host side of a render launch: the samples and record slots of the next launch as pure functions (launch_plan.h); grids,
//                          the timed-launch bracket, the loop that splits a pass into launches, the path-granular launch with its repeat (ResolvePending,
//                          SettlePending), the item launch; where a pass adds its sums is an argument (RenderSamples).  Grow, and behind it the growth of
//                          the handle's index sort (IndexSortBufs, below).  Light tracing's launches (LtTraceLaunches) with what its three entry points
//                          share: their argument checks (LtCheck) and the one repeat of a launch that outgrew its record buffer (RepeatOutgrownLaunch).
//   bvh_device_build.inc   AMBER_PT_FLAG_DEVICE_BUILD: engine BVH's tree built by kernels at create (Morton order, radix-tree hierarchy, the host builder's
//                          bounds / padding / outward binary16 planes) instead of bvh_build.h's binned-SAH build on the host.
//   bvh_update.inc         amber_hip_pt_update_objects: new object geometry into a live handle -- records converted and checked by a kernel, then the
//                          tree made valid again on the device: refitted (any tree, topology kept) or rebuilt (the Morton tree, in place).
//   ray_query.inc          amber_hip_pt_cast_rays / amber_hip_pt_occluded: the caller's rays through the handle's engine -- engine BVH in a persistent refill
//                          kernel (closest hit, and the any-hit walk BvhAnyHit), the other engines one thread per ray through ClosestHit<kEngine>;
//                          LaunchPerItem, the launch of every kernel with a thread per item (its engine front end: dev_closest_hit.h).  StagedTrips, the
//                          trips of every call with host pointers through the handle's one pair of staging buffers (HostStaging, below), and the
//                          argument checks of the three calls that answer the caller's buffers (CheckQueryCall, CheckQueryPointers).
//   path_query.inc         amber_hip_pt_trace_paths: radiance along the caller's rays -- the bounce loop of the render kernels from (origin, dir, weight, sampler
//                          state) records, a lane per ray with its samples in sequence, idle lanes refilled per ray from one counter; every engine.
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
//                          permutation sorted by (pixel, pass, path, bounce) with two stable radix sorts (the handle's IndexSortBufs, which the
//                          two files below use as well), then one thread per pixel run.
//   lt_photons.inc         amber_hip_lt_trace_photons: the vertex records of a light-tracing launch (PathShade's second sink) into the caller's buffer in
//                          (sample, path, bounce) order -- two stable radix sorts of an index permutation, one gather of the 64-byte records.
//   photon_map.inc         amber_hip_pm_build / amber_hip_pm_gather / amber_hip_pm_release: the handle's photon map -- a uniform grid over the caller's photons (bounds
//                          by a reduction, cell keys, one stable radix sort, cell starts, a packed {position, index} array and a payload array) and the
//                          k-nearest radiance gather, a lane per query: one sweep over the cells the radius touches; a bisection over the bit patterns of
//                          the squared distance for the queries that have more than k photons in radius.
//   pt_replay.inc          replay_records_kernel: the paths a scouted launch flagged (pt_megakernel's AMBER_KERNEL_SCOUT instantiation), traced again with
//                          their weights, one lane per record; scout_bound.h: the rule that flags them and the host's bound of the eye weight.
//   pt_records.inc         records {q, rgb} -> path order -> the per-pixel sums of the numerical contract (rec_rank / scan / place, reduce_flagged);
//                          pixel_mask_kernel (candidates of a pixel block's eye rays).
// LAB BUILD (-DAMBER_LAB -> libamber_hip_lab.so; include/amber_hip_lab.h): the schedulers that were measured and lost but stay provably equal
// (bvh_pool.inc, wavefront.inc, bvh_stream.inc), the known-answer kernels and entry points the tests use (lab_kernels.inc, lab_api.inc) and the
// signature instantiations of the product kernels.  libamber_hip.so is built WITHOUT it and exports only the documented ABI.  The lab's stage
// timing of the three files above is StageClock (below), which the product build compiles to nothing.
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
#include "launch_plan.h"
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
#include "pt_replay.inc"
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

// Lab build: the device time between kN events of a stage, summed per interval (ms[i]: from event i to event i + 1) until the stage's
// amber_hip_kat_*_stage_ms hook (lab_api.inc: StageMs) reports and zeroes the sums; the hook's first call switches the clock on.  A timed stage waits
// for its last event.  The product build has no clock: every member is an empty inline function, and Get leaves the event null.
template <int kN>
struct StageClock {
#ifdef AMBER_LAB
  bool on = false;
  double ms[kN - 1] = {};
  Event ev[kN];
  int Get(int i, hipEvent_t* e) {               // the event itself, for a launch code that records it (LtSink)
    if (on && !ev[i].v) HIP_TRY(hipEventCreate(&ev[i].v));
    if (on) *e = ev[i].v;
    return AMBER_OK;
  }
  int Mark(int i, hipStream_t st) {
    hipEvent_t e = nullptr;
    AMBER_TRY(Get(i, &e));
    if (e) HIP_TRY(hipEventRecord(e, st));
    return AMBER_OK;
  }
  int Lap(int first, int last) {                // the intervals between the recorded events first .. last into the sums
    if (!on) return AMBER_OK;
    HIP_TRY(hipEventSynchronize(ev[last].v));
    for (int i = first; i < last; i++) { float t = 0; HIP_TRY(hipEventElapsedTime(&t, ev[i].v, ev[i + 1].v)); ms[i] += t; }
    return AMBER_OK;
  }
#else
  int Get(int, hipEvent_t*) { return AMBER_OK; }
  int Mark(int, hipStream_t) { return AMBER_OK; }
  int Lap(int, int) { return AMBER_OK; }
#endif
};

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
// Where host pointers pass through device memory: the input and the output of the trips of amber_hip_pt_cast_rays / _occluded / _trace_paths and
// amber_hip_pm_gather (AMBER_RAYS_HOST; ray_query.inc: StagedTrips), the photons amber_hip_pm_build reads (`in`) and the sorted records of a launch
// of amber_hip_lt_trace_photons on their way out (`out`) (AMBER_PHOTONS_HOST).  Grown on first use, kept, released by amber_hip_pm_release and with
// the handle.  ONE pair serves them all because no two users can hold it at once: every user works on the handle's stream and waits for that stream
// before its call returns, none calls another, and within amber_hip_lt_trace_photons the asynchronous copy out of launch i has been waited for (every
// launch is, LtTraceLaunches) before launch i + 1's records are sorted into `out` -- and Grow waits for the stream before it frees what it replaces.
struct HostStaging { DevBuf<uint8_t> in, out; };
// The stable sort of an index permutation by 64-bit keys, in one or two passes of rocPRIM's radix sort (two: the second key is the major one) --
// the order of lt_accumulate.inc, lt_photons.inc and photon_map.inc, one at a time on the handle's stream.  Grown on first use, kept.
//   Prepare    grows everything (which may wait for the stream): before the stage's first kernel and its first timing event
//   keys()     where the caller's key kernel writes the keys of the next pass -- for the first pass with the identity in order(), for the second
//              one read through order(), the first pass's result
//   Pass(i)    sorts; afterwards order() is the permutation and sorted_keys() holds its keys
struct IndexSortBufs {
  DevBuf<unsigned long long> key[2];        // sort keys, in and out
  DevBuf<uint32_t> index[2];                // the permutation, used ping-pong
  DevBuf<uint8_t> temp;                     // rocPRIM's temporary storage
  hipStream_t stream = nullptr;             // of the sort in flight (Prepare): the handle's
  uint32_t n = 0;                           // ... its items
  unsigned int end_bit[2] = {0, 0};         // ... the bits of its passes' keys
  size_t temp_bytes[2] = {0, 0};
  int cur = 0;                              // ... and the slot of `index` that holds the current permutation
  int Prepare(amber_hip_pt* h, uint32_t n_items, unsigned int end_bit0, unsigned int end_bit1, const char* keys_label, const char* order_label);   // end_bit1 == 0: one pass; defined behind Grow (pt_launch.inc)
  unsigned long long* keys() const { return key[0].p; }
  const unsigned long long* sorted_keys() const { return key[1].p; }
  uint32_t* order() const { return index[cur].p; }
  int Pass(int i) {
    HIP_TRY(rocprim::radix_sort_pairs(temp.p, temp_bytes[i], key[0].p, key[1].p, index[cur].p, index[cur ^ 1].p, n, 0u, end_bit[i], stream));   // stable: ties stay in the order of the pass before
    cur ^= 1;
    return AMBER_OK;
  }
};
uint32_t BitsFor(uint32_t below) {            // bits that hold every value < below
  uint32_t bits = 0;
  while (bits < 32u && (below - 1u) >> bits) bits++;
  return below > 1u ? bits : 1u;
}
// amber_hip_lt_render_pass (lt_accumulate.inc): the scratch of the ordered sum, grown on first use, kept, released with the handle
struct LtAccumBufs {
  DevBuf<float4> value;                     // {rgb, pad} of the records in sorted order
  DevBuf<unsigned int> longest;             // AmberLtPassInfo.longest_run of the call in flight
  uint32_t capacity = 0;                    // records d_splats holds for that call: AMBER_LT_SPLAT_CAPACITY0, or what a launch made it grow to
  StageClock<3> clock;                      // amber_hip_kat_lt_stage_ms: sort | sum (a timed accumulation waits for the stream)
};
// amber_hip_lt_trace_photons (lt_photons.inc): nothing of it exists before the first call
struct PhotonBufs {
  DevBuf<float4> staging;                   // the records of the launch in flight in arrival order, four float4 each
  uint32_t capacity = 0;                    // records it holds: AMBER_PHOTON_CAPACITY0, or what a launch made it grow to
  DevBuf<unsigned int> count;               // slots claimed by the launch in flight
  DevBuf<unsigned long long> rays;          // casts of the call in flight: a counter of its own, the handle's is not touched
  StageClock<5> clock;                      // amber_hip_kat_photon_stage_ms: trace | (the host reads the counters) | sort | gather (waits for the stream after every launch's gather)
};
// amber_hip_pm_build / amber_hip_pm_gather (photon_map.inc): the handle's one photon map and the scratch of its build, nothing of it before the first build
struct PhotonMapBufs {
  bool built = false;                       // a build has succeeded and amber_hip_pm_release has not been called since
  AmberPhotonMapInfo info{};                // of that build (n_photons - n_dropped photons are in the map)
  DevBuf<float4> posidx;                    // {x, y, z, input index} of the kept photons in cell order: what the distance test reads
  DevBuf<float4> payload;                   // {dir_out, 0} {weight, 0} in the same order: read for the photons that pass it
  DevBuf<uint32_t> start;                   // cells + 1: the first photon of every cell
  DevBuf<uint32_t> ctl;                     // build: ordered bit patterns of the bounds (3 minima, 3 maxima), the dropped count
  StageClock<3> clock;                      // amber_hip_kat_pm_stage_ms: build | gather (events 0, 1 around a build, 1, 2 around a gather's launch, which then waits for the stream)
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
// amber_hip_pt_cast_rays / amber_hip_pt_occluded (ray_query.inc): allocated by the first query, reused by every later one
struct RayQueryBufs {
  DevBuf<int32_t> stack;                    // engine BVH: the global levels of the hybrid traversal stack, [level][thread of the largest query grid]
  uint64_t stack_threads = 0;               // ... and the threads it was allocated for
  DevBuf<unsigned int> next;                // engine BVH: the work counter
};
// Path-granular launches (pt_launch.inc: LaunchPaths, ResolvePending): bitmap, records in arrival order, measurements in path order, ranks -- and
// the launch whose record counter the host has not looked at yet
// What fills a launch's record buffer: the product's render kernel, or (lab build, amber_hip_kat_accumulate) the kernel that emits the caller's records
// -- then with its device inputs, so that a repeat of the launch finds them again.
struct RecordProducer {
  bool lab = false;
  const uint32_t* q = nullptr;              // device, n_items: the path of every item, AMBER_REC_UNUSED = the lane emits nothing
  const float* rgb = nullptr;               // device, n_items * 3
  uint32_t n_items = 0, n_waves = 0;
  unsigned long long rays = 0;              // what the launch adds to its ray counter
};
struct PathLaunchBufs {
  DevBuf<uint32_t> flags;  bool flags_dirty = true;   // dirty: must be cleared before the next launch
  DevBuf<uint32_t> touched;
  DevBuf<uint4> records;   DevBuf<float> sorted;   uint32_t rec_capacity = 0;
  DevBuf<unsigned int> launch_ctl;          // [0] queue head of the path kernels, [1] = *rec_count, [2..3] = *rays_launch
  unsigned int* rec_count = nullptr;
  unsigned long long* rays_launch = nullptr;
  DevBuf<uint32_t> excl, block_sum;
  Owned<unsigned int*, hipHostFree> h_rec_count;   // pinned: the record counter of the launch in flight
  Event pending_event;
  bool pending = false, pending_checked = true;   // a launch whose record counter has not been looked at yet; checked = it cannot have run out of slots
  uint32_t pending_first = 0, pending_n = 0;
  float* pending_target = nullptr;          // where that launch adds its sums (the framebuffer, a batch buffer): a repeat adds to the same buffer
  RecordProducer pending_producer;          // ... and what produced its records: a repeat runs the same producer
  uint64_t n_launches = 0, n_repeats = 0;   // launches reduced so far, and how many of them were repeats (amber_hip_kat_accumulate reports the difference)
  bool density_known = false;
  double rec_density = 0;                   // record slots used per path, as the last launch measured it
  DevBuf<float> carried;                    // measurements carried across bounces (degenerate paths only)
};
// amber_hip_pt_kernel_time: the render kernels between event pairs (pt_launch.inc: TimedLaunch)
struct LaunchTimer {
  std::vector<std::pair<Event, Event>> events;   // pool of event pairs, one per timed launch in flight
  size_t used = 0;
  uint32_t folded_launches = 0;             // launches already folded into folded_ms
  double folded_ms = 0;
  void reset() { used = 0; folded_launches = 0; folded_ms = 0; }
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
  RayQueryBufs query;                       // amber_hip_pt_cast_rays / amber_hip_pt_occluded
  HostStaging staging;                      // every call that takes host pointers through device memory
  IndexSortBufs sort;                       // the sorts of light tracing's accumulation, of the photons and of the photon map
  ImageStageBufs img;                       // resolve, AOVs, the filters, batches
  DevBuf<float> d_fb;
  DevBuf<unsigned long long> d_rays;
  DevBuf<unsigned int> d_next;
  DevBuf<unsigned long long> d_stamps;
  DevBuf<DevSplat> d_splats;
  DevBuf<unsigned int> d_splat_count;
  uint64_t hashed_seed_lt = 0;
  LtAccumBufs lt;                           // amber_hip_lt_render_pass
  PhotonBufs photons;                       // amber_hip_lt_trace_photons
  PhotonMapBufs pm;                         // amber_hip_pm_build / amber_hip_pm_gather
  DevBuf<float> d_partial;                  // pt_bvh_megakernel: per-item sums
  PathLaunchBufs paths;                     // the path-granular launches and the one in flight
  DevBuf<int32_t> d_bvh_stack;              // pt_bvh_pool_kernel (lab build): deep traversal-stack levels
  DevBuf<unsigned long long> d_sig;         // amber_hip_pt_signatures
  DevBuf<uint32_t> d_pixel_mask;            // two-phase engine: primary-ray candidates per band pixel
  // pixel_mask_kernel is enqueued on the render stream by create (0.07 ms since the masks are per 4 x 4 block of pixels: it no longer pays to
  // overlap it -- a second stream costs a millisecond of host time to create, more than the kernel it would hide)
  bool pixel_mask_ready = false;            // the kernel has been enqueued in front of everything that reads d_pixel_mask
  bool scout = false;                       // path launches run the weight-free scout + replay_records_kernel (DecideScout); false: the full kernel
  uint32_t scout_bound0 = 0;                // ... and the bound of this lens's eye weight that the scout starts every path with (scout_bound.h)
  int n_cus = 256;
  uint32_t row_begin = 0, row_end = 0, stripe_rows = 0, stripe_period = 0, local_rows = 0;
  uint64_t seed = 0, hashed_seed = 0;
  DevBuf<float> d_wf;                       // WAVEFRONT: queues + meas + counts in one allocation
  uint32_t n_materials = 0;
  LaunchTimer timer;                        // amber_hip_pt_kernel_time
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

int StartPixelMasks(amber_hip_pt* h, float* timing);      // defined with the launch code (pt_launch.inc)
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
#if AMBER_SCOUT
  h->scout = amber_prep::DecideScout(h->engine, h->hit_engine, params->reserved, h->lens, p.blades, p.materials, sensor->scene_width, sensor->scene_height, &h->scout_bound0);
#endif
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

#include "pt_launch.inc"

#include "ray_query.inc"
#include "path_query.inc"
#include "image_stage.inc"
#include "resolve.inc"
#include "aov.inc"
#include "denoise.inc"
#include "denoise_variance.inc"
#include "temporal.inc"
#include "lt_accumulate.inc"
#include "lt_photons.inc"
#include "photon_map.inc"

namespace {
#ifdef AMBER_LAB
int RenderPassWavefront(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples);      // lab_api.inc
#endif

// amber_hip_pt_render_pass (batch_name null: the samples are added to the framebuffer) and amber_hip_pt_render_batch (its name, which its messages begin
// with): the samples into the handle's batch buffer (zeroed) instead, then moments_fold_kernel: fb = fb + B and the batch's luminance into the moments.
int RenderBand(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples, const char* batch_name) {
  const std::string prefix = batch_name ? std::string(batch_name) + ": " : std::string();
  if (!h) return Fail(AMBER_EINVAL, prefix + "null handle");
  if (n_samples == 0) return AMBER_OK;
  if (static_cast<uint64_t>(first_sample) + n_samples > 0xffffffffull) return Fail(AMBER_EINVAL, prefix + "sample index overflow");
  HIP_TRY(hipSetDevice(h->device));
  const uint32_t n_pixels = static_cast<uint32_t>(BandPixels(h));
  if (n_pixels == 0) return AMBER_OK;                    // empty band
  if (!batch_name) {
#ifdef AMBER_LAB
    if (h->engine == AMBER_ENGINE_WAVEFRONT) return RenderPassWavefront(h, first_sample, n_samples);
#endif
    return RenderSamples(h, first_sample, n_samples, n_pixels, h->d_fb, nullptr);
  }
  if (h->engine == AMBER_ENGINE_WAVEFRONT) return Fail(AMBER_EINVAL, prefix + "not part of the lab engine WAVEFRONT");
  // a pass in flight whose record buffer was sized from an estimate may have to be repeated: it must stand before the batch buffer is zeroed behind it
  AMBER_TRY(SettlePending(h));
  AMBER_TRY(EnsureMoments(h, batch_name));
  AMBER_TRY(Grow(h, h->img.batch, static_cast<size_t>(n_pixels) * 3u, "batch sums"));
  HIP_TRY(hipMemsetAsync(h->img.batch, 0, static_cast<size_t>(n_pixels) * 3u * sizeof(float), h->stream));
  // (after a failure of the two calls below a launch may stay pending with the batch buffer for its target: a repeat of it then adds to a buffer nobody
  // reads -- the next batch zeroes it behind that repeat on the stream -- so nothing of a failed batch reaches the framebuffer or the moments)
  AMBER_TRY(RenderSamples(h, first_sample, n_samples, n_pixels, h->img.batch, nullptr));
  AMBER_TRY(SettlePending(h));                           // ... and so must the batch's own last launch before the fold reads its sums (as amber_hip_pt_resolve waits)
  return FoldBatch(h, n_samples);
}
}  // namespace

extern "C" {

int amber_hip_pt_render_pass(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples) {
  return Guarded("amber_hip_pt_render_pass", [&] { return RenderBand(h, first_sample, n_samples, nullptr); });
}

int amber_hip_pt_render_batch(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples) {
  return Guarded("amber_hip_pt_render_batch", [&] { return RenderBand(h, first_sample, n_samples, "amber_hip_pt_render_batch"); });
}

int amber_hip_lt_trace_range(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples, uint32_t path_begin, uint32_t path_end,
                             AmberSplat* out, uint32_t capacity, uint32_t* n_out, uint64_t* ray_count) { return Guarded("amber_hip_lt_trace_range", [&]() -> int {
  if (!h || !n_out || (capacity && !out)) return Fail(AMBER_EINVAL, "null argument");
  *n_out = 0;
  if (ray_count) *ray_count = 0;
  AMBER_TRY(LtCheck(h, "", "WSOP", first_sample, n_samples, path_begin, path_end));
  const uint32_t n_paths = path_end - path_begin;
  if (LtNothingToDo(h, n_samples, n_paths)) return AMBER_OK;
  HIP_TRY(hipSetDevice(h->device));
  AMBER_TRY(ResolvePending(h));
  const uint32_t dev_capacity = capacity ? capacity : 1u;
  AMBER_TRY(Grow(h, h->d_splats, dev_capacity, "splats"));
  if (!h->d_splat_count) HIP_TRY(h->d_splat_count.alloc(1));
  uint64_t total = 0;                                         // splats produced (also beyond the caller's capacity)
  unsigned long long rays_first = 0, rays_last = 0;
  bool any = false;
  const int rc = LtTraceLaunches(h, first_sample, n_samples, path_begin, n_paths, false, dev_capacity, SplatLtSink(h),
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

int amber_hip_lt_trace_photons(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples, uint32_t path_begin, uint32_t path_end, uint32_t surfaces,
                               AmberPhoton* out, uint64_t capacity, AmberPhotonInfo* info, uint32_t flags) {
  return Guarded("amber_hip_lt_trace_photons", [&] { return TracePhotons(h, first_sample, n_samples, path_begin, path_end, surfaces, out, capacity, info, flags); });
}

int amber_hip_pm_build(amber_hip_pt* h, const AmberPhoton* photons, uint64_t n, float cell_size, uint32_t flags, AmberPhotonMapInfo* info) {
  return Guarded("amber_hip_pm_build", [&] { return PmBuild(h, photons, n, cell_size, flags, info); });
}

int amber_hip_pm_gather(amber_hip_pt* h, uint64_t n, const AmberGatherQuery* q, AmberGatherResult* out, uint32_t k, uint32_t flags) {
  return Guarded("amber_hip_pm_gather", [&] { return PmGather(h, n, q, out, k, flags); });
}

int amber_hip_pm_release(amber_hip_pt* h) {
  return Guarded("amber_hip_pm_release", [&] { return PmRelease(h); });
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
  h->timer.reset();
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

int amber_hip_pt_trace_paths(amber_hip_pt* h, uint64_t n, const AmberPathRay* rays, AmberPathResult* out, uint32_t n_samples, uint32_t max_depth, uint32_t flags) {
  return Guarded("amber_hip_pt_trace_paths", [&] { return TracePaths(h, n, rays, out, n_samples, max_depth, flags); });
}

uint64_t amber_hip_sampler_state(uint64_t seed, uint32_t pixel, uint32_t sample) { return HostXorShiftSeed(HostSplitMix64(seed), pixel, sample); }

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
  const LaunchTimer& t = h->timer;
  double tot = t.folded_ms;
  for (size_t i = 0; i < t.used; i++) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, t.events[i].first.v, t.events[i].second.v));
    tot += ms;
  }
  if (n_launches) *n_launches = t.folded_launches + static_cast<uint32_t>(t.used);
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

// pt_args.h -- kernel arguments of the render kernels and the record-emission helpers they share.
// Part of the one translation unit pt_host.hip (kernels are launched from there); see its header comment.
#pragma once

struct RenderArgs {
  DevScene scene;
  float* partial;            // pt_bvh_megakernel: [n_chunks][n_pixels][3] per-item sums of this launch
  uint32_t* flags;           // path-granular kernels: bit q set = path q of this launch ended with a non-zero measurement ...
  uint32_t* touched;         // ... and bit (q / n_samples) of this one: the band pixels that have any record (the reduction skips the others)
  uint4* records;            // ... appended as {q, r, g, b}; q = 0xffffffff marks a reserved slot that was never used
  unsigned int* rec_count;   // slots handed out so far (waves reserve AMBER_REC_BLOCK at a time)
  uint32_t rec_capacity;     // slots of `records`; a launch that needs more is repeated by the host with a larger buffer
  uint32_t scout_bound0;     // pt_megakernel's scout: the host's bound of log2 |eye weight| for this lens, sixteenths of a bit (scout_bound.h).  It fills the four
                             // bytes of padding in front of the next pointer: no offset moves and the record keeps its size, so the instantiations that were there
                             // before it read their cold arguments where they did
  unsigned long long* ray_count;
  unsigned int* next_item;   // work-queue head (zeroed before every launch)
  unsigned long long* stamps; // diagnostic build only (AMBER_STAMPS): 8 section sums
  DevSplat* splats;          // light tracing: splat records, their counter and capacity
  unsigned int* splat_count;
  uint32_t splat_capacity;
  uint32_t photon_surfaces;  // amber_hip_lt_trace_photons: the AMBER_PHOTON_* mask; `splats` then holds AmberPhoton records (64 B), counter and capacity are theirs
  int32_t* bvh_stack;        // pt_bvh_pool_kernel: traversal-stack levels beyond the LDS part, [level][thread of the grid]
  float* carried;            // pt_bvh_pool_kernel: measurements of the (degenerate) paths that carry a non-zero one across bounces, [thread of the grid * kRays/64 ...]
  const uint32_t* pixel_mask; // pt_megakernel, two-phase engine: candidate mask of every band pixel's primary rays (pixel_mask_kernel); null = off
  unsigned long long* sig;   // signature variants: sig[q] = the path's hit-object / hit-distance hashes (amber_hip_pt_signatures)
  uint64_t hashed_seed;      // SplitMix64(global_seed)
  uint32_t row_begin;
  uint32_t stripe_rows, stripe_period;   // 0,0 = contiguous rows
  ExactDiv div_stripe_rows;  // lrow / stripe_rows without a divide (exact_div.h); unused when stripe_rows == 0
  ExactDiv div_width;        // plocal / scene.sensor.w
  uint32_t n_pixels;         // pixels of the band
  uint32_t first_sample, n_samples;
  uint32_t n_chunks, n_items;   // pt_bvh_megakernel: items = (pixel, chunk); path-granular kernels: n_items = paths of the launch
  ExactDiv div_samples;      // q / n_samples
  uint32_t path_offset;      // light tracing: index of the first light path of this launch's range (amber_hip_lt_trace_range)
  uint32_t shade_batch;      // pt_bvh_megakernel: lanes that must have finished their traversal before the wave shades (the handle's choice, BvhShadeBatch)

  // The divisors of the pixel bookkeeping are the same for every path of a launch: their dividers are formed here, together with the fields
  // they belong to, for every launch anew (nothing is cached: a handle's next launch may have another sample count).  SetBand reads the
  // sensor width: call it once `scene` is set.
  void SetBand(uint32_t row_begin_, uint32_t stripe_rows_, uint32_t stripe_period_) {
    row_begin = row_begin_; stripe_rows = stripe_rows_; stripe_period = stripe_period_;
    div_stripe_rows = MakeExactDiv(stripe_rows_); div_width = MakeExactDiv(scene.sensor.w);
  }
  void SetSamples(uint32_t first_sample_, uint32_t n_samples_) { first_sample = first_sample_; n_samples = n_samples_; div_samples = MakeExactDiv(n_samples_); }
};

static_assert(offsetof(RenderArgs, scout_bound0) + 4 == offsetof(RenderArgs, ray_count), "scout_bound0 sits in what was padding");

// What a bounce of a light path is handed for its records: the splat sink, or (kPhotons) the vertex sink of amber_hip_lt_trace_photons over the same
// three arguments
template <bool kPhotons>
__device__ __forceinline__ typename std::conditional<kPhotons, PhotonSink, SplatSink>::type MakeLightSink(const RenderArgs& a, uint32_t path, uint32_t sample) {
  const SplatSink splat{a.splats, a.splat_count, a.splat_capacity, path, sample, a.scene.sensor.size_f};
  if constexpr (kPhotons) return PhotonSink{splat, reinterpret_cast<float4*>(a.splats), a.photon_surfaces};
  else return splat;
}

// Local row of a band -> row of the frame: contiguous rows from row_begin (stripe_rows == 0: the divider is not used), or stripes of stripe_rows rows
// every stripe_period rows.  The kernels that read these fields as plain arguments share it through PlacePath / PlacePixel below.  Four sites keep their
// own form: pt_megakernel reads the fields cold, one by one (pt_megakernel.inc); pt_bvh_megakernel divides plainly on purpose (its comment cites the
// measurement); replay_records_kernel's instruction stream is pinned, and through PlacePath its schedule moves (EXPERIMENTS.md, device fold);
// kat_signature_kernel's frozen argument list has no divider for the width.
__device__ __forceinline__ uint32_t FrameRow(uint32_t row_begin, uint32_t stripe_rows, uint32_t stripe_period, ExactDiv div_stripe_rows, uint32_t lrow) {
  if (stripe_rows == 0u) return row_begin + lrow;
  const uint32_t band = Quotient(div_stripe_rows, lrow);
  return row_begin + band * stripe_period + (lrow - band * stripe_rows);
}
// Where a path lies: band pixel, sample offset within the launch, pixel of the frame.  Args: RenderArgs, or any record with its band fields (SetBand).
struct PathPlace { uint32_t plocal, k, px, py; };
template <typename Args>
__device__ __forceinline__ PathPlace PlacePixel(const Args& a, uint32_t plocal, uint32_t k = 0u) {
  const uint32_t lrow = Quotient(a.div_width, plocal);
  return PathPlace{plocal, k, plocal - lrow * a.scene.sensor.w, FrameRow(a.row_begin, a.stripe_rows, a.stripe_period, a.div_stripe_rows, lrow)};
}
// Path q = plocal * n_samples + k of a launch (pt_megakernel.inc)
__device__ __forceinline__ PathPlace PlacePath(const RenderArgs& a, uint32_t q) {
  const uint32_t plocal = Quotient(a.div_samples, q);
  return PlacePixel(a, plocal, q - plocal * a.n_samples);
}
// The sampler state the k-th sample of the launch at that pixel starts from: Image index x + y*W (image.h:116-124), sample first_sample + k.  k is an
// argument, not place.k: a kernel that owns a pixel (aov_kernel, wf_generate_kernel) places it once with PlacePixel and seeds every sample from it.
template <typename Args>
__device__ __forceinline__ uint64_t PathSeed(const Args& a, const PathPlace& p, uint32_t k) {
  return XorShiftSeed(a.hashed_seed, p.px + p.py * a.scene.sensor.w, a.first_sample + k);
}

// COLD kernel arguments of pt_megakernel.  A field of RenderArgs that the kernel reads as `a.field` is loaded once at the kernel's entry and then
// lives in SGPRs for the whole persistent loop; the per-bounce code needs every SGPR it can get, so the compiler parks such values in the lanes
// of a VGPR and fetches them back with v_readlane_b32 wherever they are used -- VALU instructions (plus hazard s_nops) that compute nothing, in
// a kernel bound by VALU issue.  What the every-bounce path never touches (the claim, the primary round's pixel bookkeeping, the record buffers,
// the carried measurements) is therefore read from the kernarg segment NEXT TO ITS USE, like the lens record (LoadLens): a scalar load that hits
// the constant cache once per 64 paths.  The empty asm makes the pointer opaque per use -- otherwise the loads are hoisted back out of the loop.
// Only valid in a kernel whose FIRST parameter is a by-value RenderArgs (the explicit arguments start at offset 0 of the segment).
struct ColdArgs {
  ConstWords w;
  __device__ __forceinline__ static ColdArgs Open() {
    ConstWords w = (ConstWords)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(w));
    return ColdArgs{w};
  }
  template <typename T> __device__ __forceinline__ T Get(size_t byte_offset) const {
    static_assert(sizeof(T) % 4 == 0 && alignof(T) <= 8, "whole dwords");
    union U { T value; uint32_t words[sizeof(T) / 4]; __device__ U() {} } u;
#pragma unroll
    for (unsigned k = 0; k < sizeof(T) / 4; ++k) u.words[k] = w[byte_offset / 4 + k];
    return u.value;
  }
};
#define AMBER_COLD(cold, field) (cold).Get<decltype(static_cast<const RenderArgs*>(nullptr)->field)>(offsetof(RenderArgs, field))

// FNV-1a-32 step over the four bytes of v (path signatures: amber_hip_kat_signatures, amber_hip_pt_signatures)
__device__ __forceinline__ uint32_t Fnv32(uint32_t h, uint32_t v) {
#pragma unroll
  for (int k = 0; k < 4; k++) { h ^= (v >> (8 * k)) & 0xffu; h *= 16777619u; }
  return h;
}
// A path's signature: FNV-1a-32 over the object index of every cast (0xffffffff = miss) and over the bits of every hit distance, packed {obj, t << 32}
struct PathSig {
  uint32_t obj, t;
  __device__ __forceinline__ void Reset() { obj = 2166136261u; t = 2166136261u; }          // the FNV offset basis
  __device__ __forceinline__ void Add(const Bounce& b) {
    obj = Fnv32(obj, static_cast<uint32_t>(b.object));
    if (b.object >= 0) t = Fnv32(t, __float_as_uint(b.t));
  }
  __device__ __forceinline__ unsigned long long Packed() const { return static_cast<unsigned long long>(obj) | (static_cast<unsigned long long>(t) << 32); }
};

// Accumulation without owners, device side.  A path that ends with a measurement other than +0 appends {q, rgb} to the
// record buffer and sets bit q.  Slots are reserved per WAVE, AMBER_REC_BLOCK at a time (one atomicAdd on the shared
// counter per 64 records: a scene in which every second path reaches a light would otherwise put 5e8 atomics on one
// address -- the L2 retires ~88 of those per microsecond); [rec_next, rec_end) is the wave's open block (SGPRs).  Must be
// called with all 64 lanes active.  A slot beyond the buffer is not written: the counter then tells the host to repeat
// the launch with a larger buffer (RenderPassPaths).
#define AMBER_REC_BLOCK 64u
#define AMBER_REC_UNUSED 0xffffffffu
// The buffers are handed over by a callable that is asked for them only when the wave has a record to write (pt_megakernel: cold arguments).
struct RecordSink { uint4* records; uint32_t* flags; uint32_t* touched; unsigned int* rec_count; uint32_t rec_capacity; ExactDiv div_samples; };
template <typename SinkOf>
__device__ __forceinline__ void EmitRecords(SinkOf sink_of, bool emit, uint32_t q, V3 meas, uint32_t& rec_next, uint32_t& rec_end) {
  const unsigned long long me = __ballot(emit);
  if (me == 0ull) return;                                     // wave-uniform
  const RecordSink a = sink_of();
  const uint32_t n = static_cast<uint32_t>(__popcll(me));
  const uint32_t rank = WaveRank(me);
  const uint32_t room = rec_end - rec_next;
  uint32_t fresh = 0;
  if (n > room) {                                             // n <= 64 = AMBER_REC_BLOCK: one new block always suffices
    if ((threadIdx.x & 63u) == 0u) fresh = atomicAdd(a.rec_count, AMBER_REC_BLOCK);
    fresh = __builtin_amdgcn_readfirstlane(fresh);
  }
  if (emit) {
    const uint32_t slot = rank < room ? rec_next + rank : fresh + (rank - room);
    if (slot < a.rec_capacity) a.records[slot] = make_uint4(q, __float_as_uint(meas.x), __float_as_uint(meas.y), __float_as_uint(meas.z));
    atomicOr(a.flags + (q >> 5), 1u << (q & 31u));
    const uint32_t p = Quotient(a.div_samples, q);
    atomicOr(a.touched + (p >> 5), 1u << (p & 31u));
  }
  if (n > room) { rec_next = fresh + (n - room); rec_end = fresh + AMBER_REC_BLOCK; }
  else rec_next += n;
}
__device__ __forceinline__ void EmitRecords(const RenderArgs& a, bool emit, uint32_t q, V3 meas, uint32_t& rec_next, uint32_t& rec_end) {
  EmitRecords([&]() { return RecordSink{a.records, a.flags, a.touched, a.rec_count, a.rec_capacity, a.div_samples}; }, emit, q, meas, rec_next, rec_end);
}
// At the end of a wave: the slots of its open block that were never used are marked.
__device__ __forceinline__ void CloseRecords(const RenderArgs& a, uint32_t rec_next, uint32_t rec_end) {
  const uint32_t k = rec_next + (threadIdx.x & 63u);
  if (k < rec_end && k < a.rec_capacity) a.records[k].x = AMBER_REC_UNUSED;
}


// path_query.inc -- amber_hip_pt_trace_paths: radiance along the caller's own rays -- the render kernels' bounce loop (PathStep / PathShade of
// dev_shading.h) started from (origin, dir, weight, sampler state) records instead of camera pixels.  Part of the one translation unit pt_host.hip;
// the device functions are the render kernels', the launch is ray_query.inc's LaunchPerItem (its grid rules, CheckRefStack).
//
//   path_query_kernel<kEngine>   A LANE OWNS ONE RAY and runs its n_samples paths in order: the sum is the sequential definition of include/amber_hip.h
//                                by construction, a result is written once, no atomics on results.  The items differ in length by two orders of
//                                magnitude (a miss is one cast, a refraction chain runs past 100), so lanes are refilled PER RAY: persistent waves claim
//                                blocks of AMBER_PATH_CLAIM rays from one counter and hand the next ray to each idle lane by ballot + mbcnt rank once
//                                AMBER_QUERY_REFILL lanes of the wave are idle or none has work (the pattern of bvh_query_kernel); every trip of the loop
//                                is one bounce of every lane that holds a ray.  The two-phase image is staged once per workgroup, before anything diverges.
//                                Engine BVH: ClosestHitBvh<true> (the one-shot per-lane traversal with the whole AMBER_BVH_STACK levels in LDS; an origin
//                                outside the scene's bounding sphere and a stack overflow take the leaf-list scan) + PathShade, on the query grid at
//                                AMBER_QUERY_WAVES; the other engines PathStep<BounceCfg<kEngine>> on the render kernels' grid (REFERENCE_BVH: one global stack
//                                column per thread of THAT grid).  The IsNanRay guard applies to the first cast of a path only: every later ray is the path's own.
//                                A ray is four 16-byte loads (the first three again at the start of each further sample: nothing of the start is kept in
//                                registers across a path), a result two 16-byte stores.
// The A/B baseline -- one thread per ray in a grid-stride loop, finished lanes waiting for their wave as in aov_kernel, behind a macro -- lost on both
// workloads (1024 x 1024 eye rays, 8 samples: Cornell through TWO_PHASE 1.726 ms against 1.473, 1M spheres through BVH 12.947 ms against 7.314;
// profiles/path_queries.txt, EXPERIMENTS.md) and was deleted.
#ifndef AMBER_PATH_CLAIM
#define AMBER_PATH_CLAIM 64u
#endif

namespace {

struct PathQueryArgs {
  DevScene scene;                                 // by value: the call's max_depth replaces scene.max_depth in this copy only
  const float4* rays;                             // AmberPathRay: {origin, pad} {dir, pad} {weight, pad} {rng_state, pad}
  float4* out;                                    // AmberPathResult: {rgb, casts} {rng_state, 0, 0}
  unsigned int* next;                             // the work counter (zeroed in front of the launch)
  uint32_t n, n_samples;
};

// What a lane holds of its ray: the path in flight, the sums of the finished samples, the sampler stream.
struct PathLane {
  PathRay path;                                   // (path.casts: the casts of the path in flight)
  V3 sum;
  uint32_t ray, sample, casts;
  bool first;                                     // the next cast is the first of its path: the caller's own ray
};

// A path of the lane's ray starts: (origin, dir, weight) as the caller gave them, measurement +0, no origin object
__device__ __forceinline__ void PathQueryStart(const float4* __restrict__ rays, PathLane& p) {
  const float4 ro = rays[4u * static_cast<size_t>(p.ray)], rd = rays[4u * static_cast<size_t>(p.ray) + 1u], rw = rays[4u * static_cast<size_t>(p.ray) + 2u];
  p.path.o = v3(ro.x, ro.y, ro.z); p.path.d = v3(rd.x, rd.y, rd.z); p.path.w = v3(rw.x, rw.y, rw.z);
  p.path.meas = v3(0.f, 0.f, 0.f); p.path.casts = 0u; p.path.origin_slot = -1; p.first = true;
}
__device__ __forceinline__ void PathQueryBegin(const float4* __restrict__ rays, uint32_t ray, PathLane& p) {
  p.ray = ray; p.sample = 0u; p.casts = 0u; p.sum = v3(0.f, 0.f, 0.f);
  const float4 rs = rays[4u * static_cast<size_t>(ray) + 3u];
  p.path.rng = static_cast<uint64_t>(__float_as_uint(rs.x)) | (static_cast<uint64_t>(__float_as_uint(rs.y)) << 32);
  if (p.path.rng == 0ull) p.path.rng = 0x9E3779B97F4A7C15ull;            // a zero xorshift state draws 0 forever
  PathQueryStart(rays, p);
}

// One bounce of the lane's path; when it ends the path, the sample's sums, and after the last sample the result.  Returns false when the ray is done.
template <int kEngine>
__device__ __forceinline__ bool PathQueryBounce(const PathQueryArgs& a, const EngineLds& lds, PathLane& p) {
  const DevScene& sc = a.scene;
  bool alive;
  if (p.first && IsNanRay(p.path.o, p.path.d)) {              // misses, as in cast_rays: the cast is counted, nothing is drawn
    p.path.casts++; alive = false;
  } else if constexpr (kEngine == ENGINE_BVH) {
    HitRec h;
    ClosestHitBvh<true>(sc, lds.stack, p.path.o, p.path.d, h);
#ifdef AMBER_STAMPS
    StampCtx stamp_store{}; StampCtx* stamp_ctx = &stamp_store;
#endif
    alive = PathShade<BounceCfg<ENGINE_BVH>>(sc, lds.objects, h, p.path, BounceExtras{} AMBER_STAMP_ARG);
  } else {
#ifdef AMBER_STAMPS
    StampCtx stamp_store{}; StampCtx* stamp_ctx = &stamp_store;
#endif
    alive = PathStep<BounceCfg<kEngine>>(sc, lds, p.path, BounceExtras{} AMBER_STAMP_ARG);
  }
  p.first = false;
  if (alive) return true;
  p.sum = p.sum + p.path.meas; p.casts += p.path.casts;
  if (++p.sample < a.n_samples) { PathQueryStart(a.rays, p); return true; }
  a.out[2u * static_cast<size_t>(p.ray)] = make_float4(p.sum.x, p.sum.y, p.sum.z, __uint_as_float(p.casts));
  a.out[2u * static_cast<size_t>(p.ray) + 1u] = make_float4(__uint_as_float(static_cast<uint32_t>(p.path.rng)), __uint_as_float(static_cast<uint32_t>(p.path.rng >> 32)), 0.f, 0.f);
  return false;
}

template <int kEngine>
__global__ void __launch_bounds__(256, kEngine == ENGINE_BVH ? AMBER_QUERY_WAVES : 1) path_query_kernel(const PathQueryArgs a) {
  const EngineLds lds = StageEngineLds<kEngine, AMBER_BVH_STACK>(a.scene);   // (ends with a barrier where it stages: before anything diverges)
  PathLane p;
  p.path.o = v3(0.f, 0.f, 0.f); p.path.d = v3(0.f, 0.f, 1.f); p.path.w = p.path.o; p.path.meas = p.path.o; p.sum = p.path.o;
  p.path.rng = 1ull; p.ray = 0u; p.sample = 0u; p.path.casts = 0u; p.casts = 0u; p.path.origin_slot = -1; p.first = false;
  bool has = false;
  const uint32_t lane = threadIdx.x & 63u;
  WaveClaim claim;
  for (;;) {
    const unsigned long long m_has = __ballot(has);
    const uint32_t n_idle = 64u - static_cast<uint32_t>(__popcll(m_has));
    if (n_idle >= AMBER_QUERY_REFILL || m_has == 0ull) {                  // wave-uniform: serve the idle lanes
      uint32_t ray = 0;
      if (ServeLanes<AMBER_PATH_CLAIM>(claim, a.next, a.n, lane, !has, ray)) { PathQueryBegin(a.rays, ray, p); has = true; }
      if (__ballot(has) == 0ull) break;
    }
    if (has) has = PathQueryBounce<kEngine>(a, lds, p);
  }
}

static_assert(sizeof(AmberPathRay) == 64 && sizeof(AmberPathResult) == 32, "a path ray is four float4, a result two");
constexpr uint64_t kPathStageRays = 1ull << 19;           // AMBER_RAYS_HOST: rays per trip through the staging buffers (32 MiB + 16 MiB)
constexpr uint32_t kPathMaxSamples = 65536u;

// One launch over n rays in device memory.  The work counter is ray_query.inc's (every query of a handle is ordered on its stream).
int LaunchPathQuery(amber_hip_pt* h, uint64_t n, const float4* d_rays, float4* d_out, uint32_t n_samples, uint32_t max_depth) {
  if (!h->query.next) HIP_TRY(h->query.next.alloc(1));
  HIP_TRY(hipMemsetAsync(h->query.next, 0, sizeof(unsigned int), h->stream));
  PathQueryArgs a{};
  a.scene = h->scene; a.rays = d_rays; a.out = d_out; a.next = h->query.next.p; a.n = static_cast<uint32_t>(n); a.n_samples = n_samples;
  if (max_depth) a.scene.max_depth = max_depth;
  return LaunchPerItem(h, n, [&](auto engine, uint32_t n_blocks) {
    hipLaunchKernelGGL((path_query_kernel<decltype(engine)::value>), dim3(n_blocks), dim3(256), 0, h->stream, a);
  });
}

int TracePaths(amber_hip_pt* h, uint64_t n, const AmberPathRay* rays, AmberPathResult* out, uint32_t n_samples, uint32_t max_depth, uint32_t flags) {
  const std::string prefix = "amber_hip_pt_trace_paths: ";
  AMBER_TRY(CheckQueryCall(h, prefix, flags, AMBER_RAYS_HOST, n, "rays"));
  if (n_samples > kPathMaxSamples) return Fail(AMBER_EINVAL, prefix + "more than 65536 samples in one call");
  if (n == 0 || n_samples == 0) return AMBER_OK;
  AMBER_TRY(CheckQueryPointers(prefix, rays, out, "rays"));
  AMBER_TRY(RefuseWideBuild(prefix));
  HIP_TRY(hipSetDevice(h->device));
  if (!(flags & AMBER_RAYS_HOST)) return LaunchPathQuery(h, n, reinterpret_cast<const float4*>(rays), reinterpret_cast<float4*>(out), n_samples, max_depth);
  return StagedTrips(h, n, kPathStageRays, sizeof(AmberPathRay), sizeof(AmberPathResult), rays, out, "path ray staging", [&](uint64_t part, uint8_t* d_in, uint8_t* d_out) {
    return LaunchPathQuery(h, part, reinterpret_cast<const float4*>(d_in), reinterpret_cast<float4*>(d_out), n_samples, max_depth);
  });
}

uint64_t HostXorShiftSeed(uint64_t hashed_global_seed, uint32_t pixel, uint32_t sample) {     // dev_math.h's XorShiftSeed on the host
  const uint64_t s = HostSplitMix64(hashed_global_seed ^ ((static_cast<uint64_t>(pixel) << 32) | sample));
  return s ? s : 0x9E3779B97F4A7C15ull;
}

}  // namespace

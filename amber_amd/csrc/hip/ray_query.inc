// ray_query.inc -- amber_hip_pt_cast_rays / amber_hip_pt_occluded: the caller's own rays through the handle's closest-hit engine (Scene::Cast and
// the visibility test built on it), in both builds.  Part of the one translation unit pt_host.hip; the device functions are the render kernels'.
//
//   bvh_query_kernel<kAnyHit>        engine BVH.  The shape of bvh_trace_rate_kernel (bvh_stream.inc, the lab's traversal-only measurement):
//                                    persistent waves claim blocks of 256 rays from one counter, idle lanes are refilled by ballot + mbcnt rank once
//                                    AMBER_QUERY_REFILL of a wave's lanes are idle, the walk is BvhRoundOn / BvhAnyHit on the hybrid LDS + global stack.
//                                    Beyond the measurement: a ray is two float4 loads with t_max in origin.w, t_max is the walk's initial bound
//                                    (BvhBeginBounded), the scene index is looked up once for the winner, ResolveHit gives position and normal, and a
//                                    result is one 32-byte record (closest hit) or one byte (any hit).  A ray whose origin lies outside the scene's
//                                    bounding sphere is answered by the leaf-list scan (BvhOriginInRange, dev_bvh.h: the tree's boxes are conservative
//                                    for origins within the scene only), through the path a traversal stack overflow takes.
//   ray_query_kernel<kEngine, kAnyHit>  LIST, TWO_PHASE, TWO_PHASE_N, REFERENCE_BVH: one thread per ray through ClosestHit<kEngine>, as the known-answer
//                                    kernel does it -- object loops wave-uniform, the two-phase image staged once per workgroup, no premask -- in a grid
//                                    no larger than the render kernels' (REFERENCE_BVH's traversal stack has one column per thread of THAT grid), each
//                                    thread taking every gridDim.x * 256-th ray.  Occlusion is the closest hit compared with t_max.
// Waves per SIMD and refill threshold: the traversal-only kernel measured 4, 5, 6 and 8 waves per SIMD equal within noise and is driven with 5 waves,
// 24 LDS stack levels and a threshold of 16 (EXPERIMENTS.md, engine BVH, round 3); these kernels take that point.  No tuning surface.
#ifndef AMBER_QUERY_WAVES
#define AMBER_QUERY_WAVES 5
#endif
#define AMBER_QUERY_LDS_LEVELS 24
#define AMBER_QUERY_REFILL 16u

namespace {

__device__ __forceinline__ void StoreRayHit(float4* __restrict__ hits, size_t i, float t, int32_t object, V3 pos, V3 nrm) {   // AmberRayHit: 32 bytes, two 16-byte stores
  hits[2u * i] = make_float4(t, __int_as_float(object), pos.x, pos.y);
  hits[2u * i + 1u] = make_float4(pos.z, nrm.x, nrm.y, nrm.z);
}
__device__ __forceinline__ void StoreRayMiss(float4* __restrict__ hits, size_t i) {
  StoreRayHit(hits, i, __builtin_nanf(""), -1, v3(0.f, 0.f, 0.f), v3(0.f, 0.f, 0.f));
}

template <bool kAnyHit>
__global__ void __launch_bounds__(256, AMBER_QUERY_WAVES) bvh_query_kernel(const DevScene sc, uint32_t n, const float4* __restrict__ rays, float4* __restrict__ hits,
                                                                           uint8_t* __restrict__ occluded, unsigned int* next, int32_t* gstack, uint32_t gstack_stride) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  __shared__ int32_t lds_stack[AMBER_QUERY_LDS_LEVELS * 256];
  const BvhStackHybrid stack{(LdsInts)(lds_stack + wave * (AMBER_QUERY_LDS_LEVELS * 64)), (GlobalInts)(gstack + (blockIdx.x * 256u + wave * 64u)), gstack_stride,
                             AMBER_QUERY_LDS_LEVELS, AMBER_BVH_STACK};
  WaveClaim claim;
  bool has = false;
  uint32_t ray_id = 0;
  V3 o = v3(0.f, 0.f, 0.f), d = v3(0.f, 0.f, 1.f);
  float t_max = 0.f;
  BvhTrav tr; HitRec hit;
  BvhIdle(tr, hit);
  for (;;) {
    const unsigned long long m_has = __ballot(has);
    const uint32_t n_idle = 64u - static_cast<uint32_t>(__popcll(m_has));
    if (n_idle >= AMBER_QUERY_REFILL || m_has == 0ull) {                  // wave-uniform: serve the idle lanes
      if (ServeLanes<256u>(claim, next, n, lane, !has, ray_id)) {
        const float4 ro = rays[2u * static_cast<size_t>(ray_id)], rd = rays[2u * static_cast<size_t>(ray_id) + 1u];   // AmberRay: origin, t_max | dir, pad
        o = v3(ro.x, ro.y, ro.z); d = v3(rd.x, rd.y, rd.z); t_max = ro.w;
        BvhBeginBounded(sc, o, d, t_max, tr, hit);
        if (tr.cur != AMBER_BVH_DONE && !BvhOriginInRange(sc, o)) { tr.cur = AMBER_BVH_DONE; tr.overflow = true; }   // the tree does not cover this origin: the scan below
        has = true;
      }
      if (__ballot(has) == 0ull) break;
    }
    if (has) {
      if constexpr (kAnyHit) {
        if (!BvhAnyHit(sc, stack, o, d, tr, hit)) {
          occluded[ray_id] = (tr.overflow ? AnyHitLeafList(sc, o, d, t_max) : hit.slot >= 0) ? 1 : 0;
          has = false;
        }
      } else {
        if (!BvhRoundOn(sc, stack, o, d, tr, hit)) {
          if (tr.overflow) ClosestHitLeafList(sc, o, d, hit);               // (unbounded: the comparison below is the filter)
          if (hit.slot >= 0 && hit.t <= t_max) {
            BvhResolveIndex(sc, hit);
            V3 pos, nrm; uint32_t mat;
            ResolveHit(sc.bvh_objects, hit, o, d, pos, nrm, mat);
            StoreRayHit(hits, ray_id, hit.t, hit.idx, pos, nrm);
          } else {
            StoreRayMiss(hits, ray_id);
          }
          has = false;
        }
      }
    }
  }
}

template <int kEngine, bool kAnyHit>
__global__ void __launch_bounds__(256) ray_query_kernel(const DevScene sc, uint64_t n, const float4* __restrict__ rays, float4* __restrict__ hits, uint8_t* __restrict__ occluded) {
  const EngineLds lds = StageEngineLds<kEngine, 1>(sc);          // (never engine BVH: no traversal stack)
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * 256u; base < n; base += static_cast<uint64_t>(gridDim.x) * 256u) {   // uniform over the workgroup
    const uint64_t i = base + threadIdx.x;
    const uint64_t k = ClampToLastItem(i, n);
    const float4 ro = rays[2u * k], rd = rays[2u * k + 1u];
    const V3 o = v3(ro.x, ro.y, ro.z), d = v3(rd.x, rd.y, rd.z);
    const float t_max = ro.w;
    HitRec h;
#ifdef AMBER_STAMPS
    StampCtx stamp_store{}; StampCtx* stamp_ctx = &stamp_store;
#endif
    ClosestHit<kEngine>(sc, lds.objects, lds.stack, o, d, -1, h AMBER_STAMP_ARG);
    if (i >= n) continue;
    const bool found = h.idx >= 0 && !IsNanRay(o, d) && h.t <= t_max;
    if constexpr (kAnyHit) {
      occluded[i] = found ? 1 : 0;
    } else if (found) {
      V3 pos, nrm; uint32_t mat;
      ResolveHit<kEngine>(sc, lds.objects, h, o, d, pos, nrm, mat);
      StoreRayHit(hits, i, h.t, h.idx, pos, nrm);
    } else {
      StoreRayMiss(hits, i);
    }
  }
}

static_assert(sizeof(AmberRay) == 32 && sizeof(AmberRayHit) == 32, "a ray and a hit are two float4 each");
constexpr uint64_t kQueryMaxRays = 1ull << 31;
constexpr uint64_t kQueryStageRays = 1ull << 20;          // AMBER_RAYS_HOST: rays per trip through the staging buffers (32 MiB + 32 MiB)

// Engine BVH's query grid at its largest: AMBER_QUERY_WAVES workgroups per CU (the launch bounds of bvh_query_kernel and aov_kernel<ENGINE_BVH>).
uint32_t QueryGridCap(const amber_hip_pt* h) { return static_cast<uint32_t>(h->n_cus) * static_cast<uint32_t>(AMBER_QUERY_WAVES); }

// One launch of a kernel with a thread per item (ray, band pixel), instantiated for the handle's engine by launch(engine, n_blocks).  The grid is no larger than
// the render kernels' (REFERENCE_BVH's traversal stack has one column per thread of THAT grid); engine BVH, whose per-item kernels keep their stacks in LDS, takes its query grid.
template <typename F>
int LaunchPerItem(amber_hip_pt* h, uint64_t n_items, F&& launch) {
  const uint32_t n_blocks = h->hit_engine == AMBER_ENGINE_BVH ? BlocksFor(n_items, QueryGridCap(h)) : PersistentBlocks(h, n_items);
  AMBER_TRY(CheckRefStack(h, n_blocks));
  WithHitEngine(h->hit_engine, [&](auto engine) -> int { launch(engine, n_blocks); return AMBER_OK; });
  HIP_TRY(hipGetLastError());
  return AMBER_OK;
}

// AMBER_RAYS_HOST: n items through the handle's staging buffers (HostStaging), at most per_trip of them at a time, and back before the call returns.
// Per trip launch(part, d_in, d_out) answers `part` records of in_size bytes at d_in with records of out_size bytes at d_out, on the handle's stream.
// `what` names the staging in an out-of-memory message.
template <typename F>
int StagedTrips(amber_hip_pt* h, uint64_t n, uint64_t per_trip, size_t in_size, size_t out_size, const void* in, void* out, const char* what, F&& launch) {
  HostStaging& s = h->staging;
  const uint64_t chunk = n < per_trip ? n : per_trip;
  AMBER_TRY(Grow(h, s.in, chunk * in_size, what));
  AMBER_TRY(Grow(h, s.out, chunk * out_size, what));
  for (uint64_t done = 0; done < n; done += chunk) {
    const uint64_t part = n - done < chunk ? n - done : chunk;
    HIP_TRY(hipMemcpyAsync(s.in.p, static_cast<const uint8_t*>(in) + done * in_size, part * in_size, hipMemcpyHostToDevice, h->stream));
    AMBER_TRY(launch(part, s.in.p, s.out.p));
    HIP_TRY(hipMemcpyAsync(static_cast<uint8_t*>(out) + done * out_size, s.out.p, part * out_size, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  return AMBER_OK;
}

// The front matter of the calls that answer the caller's buffers (rays, path rays, gather queries): the handle, the flag bits, the count ...
int CheckQueryCall(const amber_hip_pt* h, const std::string& prefix, uint32_t flags, uint32_t known_flags, uint64_t n, const char* items) {
  if (!h) return Fail(AMBER_EINVAL, prefix + "null handle");
  if (flags & ~known_flags) return Fail(AMBER_EINVAL, prefix + "unknown flag bits");
  if (n > kQueryMaxRays) return Fail(AMBER_EINVAL, prefix + "more than 2^31 " + items + " in one call");
  return AMBER_OK;
}
// ... and, once there is something to do, the two pointers
int CheckQueryPointers(const std::string& prefix, const void* in, const void* out, const char* items) {
  if (!in || !out) return Fail(AMBER_EINVAL, prefix + "null " + items + " or output pointer");
  return AMBER_OK;
}
int RefuseWideBuild(const std::string& prefix) {
#if AMBER_BVH_WIDE
  return Fail(AMBER_EINVAL, prefix + "not part of an AMBER_BVH_WIDE measurement build");
#endif
  return AMBER_OK;
}

// One launch over n rays in device memory.  Engine BVH's scratch (the global levels of the hybrid stack for the largest grid, the work counter)
// is allocated by the first query and kept.
int LaunchRayQuery(amber_hip_pt* h, uint64_t n, const float4* d_rays, void* d_out, bool any_hit) {
  float4* hits = any_hit ? nullptr : static_cast<float4*>(d_out);
  uint8_t* occluded = any_hit ? static_cast<uint8_t*>(d_out) : nullptr;
  if (h->hit_engine == AMBER_ENGINE_BVH) {
    const uint32_t max_blocks = QueryGridCap(h);
    if (!h->query.stack) {
      const hipError_t e = h->query.stack.alloc(static_cast<size_t>(max_blocks) * 256u * (AMBER_BVH_STACK - AMBER_QUERY_LDS_LEVELS));
      if (e != hipSuccess) return Fail(AMBER_ENOMEM, std::string("hipMalloc(query traversal stacks): ") + hipGetErrorString(e));
      h->query.stack_threads = static_cast<uint64_t>(max_blocks) * 256u;
    }
    if (!h->query.next) HIP_TRY(h->query.next.alloc(1));
    const uint32_t n_blocks = BlocksFor(n, max_blocks);
    if (static_cast<uint64_t>(n_blocks) * 256u > h->query.stack_threads)
      return Fail(AMBER_EINVAL, "ray query: a grid of " + std::to_string(n_blocks) + " workgroups outgrows the traversal stack (" + std::to_string(h->query.stack_threads) + " threads)");
    HIP_TRY(hipMemsetAsync(h->query.next, 0, sizeof(unsigned int), h->stream));
    const uint32_t stride = static_cast<uint32_t>(h->query.stack_threads);
    if (any_hit) hipLaunchKernelGGL(bvh_query_kernel<true>, dim3(n_blocks), dim3(256), 0, h->stream, h->scene, static_cast<uint32_t>(n), d_rays, hits, occluded, h->query.next.p, h->query.stack.p, stride);
    else hipLaunchKernelGGL(bvh_query_kernel<false>, dim3(n_blocks), dim3(256), 0, h->stream, h->scene, static_cast<uint32_t>(n), d_rays, hits, occluded, h->query.next.p, h->query.stack.p, stride);
    HIP_TRY(hipGetLastError());
    return AMBER_OK;
  }
  return LaunchPerItem(h, n, [&](auto engine, uint32_t n_blocks) {
    constexpr int kEngine = decltype(engine)::value;
    if constexpr (kEngine != ENGINE_BVH) {                    // (engine BVH has the kernel above: no ray_query_kernel<ENGINE_BVH, ..>)
      if (any_hit) hipLaunchKernelGGL((ray_query_kernel<kEngine, true>), dim3(n_blocks), dim3(256), 0, h->stream, h->scene, n, d_rays, hits, occluded);
      else hipLaunchKernelGGL((ray_query_kernel<kEngine, false>), dim3(n_blocks), dim3(256), 0, h->stream, h->scene, n, d_rays, hits, occluded);
    }
  });
}

int RayQuery(amber_hip_pt* h, uint64_t n, const AmberRay* rays, void* out, uint32_t flags, bool any_hit, const char* name) {
  const std::string prefix = std::string(name) + ": ";
  AMBER_TRY(CheckQueryCall(h, prefix, flags, AMBER_RAYS_HOST, n, "rays"));
  if (n == 0) return AMBER_OK;
  AMBER_TRY(CheckQueryPointers(prefix, rays, out, "rays"));
  AMBER_TRY(RefuseWideBuild(prefix));
  HIP_TRY(hipSetDevice(h->device));
  if (!(flags & AMBER_RAYS_HOST)) return LaunchRayQuery(h, n, reinterpret_cast<const float4*>(rays), out, any_hit);
  return StagedTrips(h, n, kQueryStageRays, sizeof(AmberRay), any_hit ? 1u : sizeof(AmberRayHit), rays, out, "ray staging", [&](uint64_t part, uint8_t* d_in, uint8_t* d_out) {
    return LaunchRayQuery(h, part, reinterpret_cast<const float4*>(d_in), d_out, any_hit);
  });
}

}  // namespace

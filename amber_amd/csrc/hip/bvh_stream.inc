// bvh_stream.inc -- traversal on its own (LAB BUILD ONLY; included by pt_host.hip under -DAMBER_LAB).
//
// bvh_trace_rate_kernel: engine BVH's resumable traversal (BvhRoundOn: the same device functions as the render kernels) with
// NOTHING else in the kernel -- persistent waves pull rays from an array, a lane that finishes writes (t, slot) and takes the
// next ray.  It answers a question of round 3 (EXPERIMENTS.md, engine BVH): how fast is this traversal when it does not share its
// register allocation (and therefore its occupancy) with shading, and how does that scale with waves per SIMD?
// Measurement and known-answer entry point (amber_hip_kat_traversal_rate), not a render path.
template <int kWaves, int kLdsLevels>
__global__ void __launch_bounds__(256, kWaves) bvh_trace_rate_kernel(const DevScene sc, uint32_t n, const float4* __restrict__ rays, float2* __restrict__ out,
                                                                     unsigned int* next, int32_t* gstack, uint32_t refill_min, uint32_t n_unique,
                                                                     uint32_t* __restrict__ rounds_out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  __shared__ int32_t lds_stack[kLdsLevels * 256];
  const BvhStackHybrid stack{(LdsInts)(lds_stack + wave * (kLdsLevels * 64)), (GlobalInts)(gstack + (blockIdx.x * 256u + wave * 64u)), gridDim.x * 256u,
                             kLdsLevels, AMBER_BVH_STACK};
  WaveClaim claim;
  bool has = false;
  uint32_t ray_id = 0, rounds = 0;
  V3 o = v3(0.f, 0.f, 0.f), d = v3(0.f, 0.f, 1.f);
  BvhTrav tr; HitRec hit;
  BvhIdle(tr, hit);
  for (;;) {
    const unsigned long long m_has = __ballot(has);
    const uint32_t n_idle = 64u - static_cast<uint32_t>(__popcll(m_has));
    if (n_idle >= refill_min || m_has == 0ull) {                          // wave-uniform: serve the idle lanes
      if (ServeLanes<256u>(claim, next, n, lane, !has, ray_id)) {
        const uint32_t src = ray_id % n_unique;                             // the ray array is walked `repeats` times: longer launches from the same rays
        const float4 ro = rays[2u * src], rd = rays[2u * src + 1u];
        o = v3(ro.x, ro.y, ro.z); d = v3(rd.x, rd.y, rd.z);
        BvhBegin(sc, o, d, tr, hit);
        has = true; rounds = 0;
      }
      if (__ballot(has) == 0ull) break;
    }
    if (has) {
      const bool more = BvhRoundOn(sc, stack, o, d, tr, hit);
      rounds++;
      if (!more) {
        if (tr.overflow) ClosestHitLeafList(sc, o, d, hit);
        out[ray_id % n_unique] = make_float2(hit.t, __int_as_float(hit.slot));
        if (rounds_out) rounds_out[ray_id % n_unique] = rounds;          // wave rounds this ray was in flight for (diagnostic)
        has = false;
      }
    }
  }
}

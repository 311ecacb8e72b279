// aov.inc -- amber_hip_pt_aov_pass / _aov_clear / _aov_download / amber_hip_pt_device_aov: the first-hit guide images of the band (albedo, depth,
// shading normal, coverage), summed over samples on the device.  Part of the one translation unit pt_host.hip; the device functions are the render
// kernels': GenerateEyeRay with the render kernels' seed, draw order and origin_slot, ClosestHit<kEngine>, ResolveHit.  The buffer and its clear,
// download and device pointer are a BandBuf of image_stage.inc; this file holds the kernel and the pass.
//
//   aov_kernel<kEngine>   ONE THREAD PER BAND PIXEL, looping over the samples first_sample .. first_sample + n_samples - 1 in this order.  The eight
//                         sums (AmberAovPixel: two float4) live in registers: read once, one binary32 addition per component and hit, written once.
//                         No sort, no atomics: the sums are the sequential definition of include/amber_hip.h by construction, and a pass over
//                         [a, a + m + n) leaves the bits of the two passes [a, a + m), [a + m, a + m + n).
//                         LIST, TWO_PHASE, TWO_PHASE_N, REFERENCE_BVH as ray_query_kernel runs them, on the front end they share (dev_closest_hit.h:
//                         StageEngineLds, ClampToLastItem; LaunchPerItem's grid), each thread taking every gridDim.x * 256-th pixel.  Engine BVH: the one-shot
//                         per-lane traversal of pt_megakernel<ENGINE_BVH> with the whole AMBER_BVH_STACK levels in LDS, so a tree of any depth the builders
//                         emit is walked; a stack overflow, and an origin outside the scene's bounding sphere, take the leaf-list scan (ClosestHitBvh<true>).
// Parallelism is the band's pixel count: a band of few pixels with many samples keeps few lanes busy however long the pass is.  That is accepted --
// guide images are taken at a handful of samples over a whole frame, where every CU has work.
// Waves per SIMD: engine BVH takes the point of the ray queries (AMBER_QUERY_WAVES = 5: five workgroups of 32 KiB of LDS stack fill a CU's 160 KiB);
// the other engines leave the registers to the compiler, as ray_query_kernel does.  No tuning surface.
namespace {

struct AovArgs {
  DevScene scene;
  float4* aov;                                    // AmberAovPixel per band pixel: {albedo.rgb, depth} {normal.xyz, coverage}
  uint64_t hashed_seed;
  uint32_t n_pixels, first_sample, n_samples;
  uint32_t row_begin, stripe_rows, stripe_period;
  ExactDiv div_stripe_rows, div_width;            // lrow / stripe_rows (unused when 0), plocal / scene.sensor.w: exact dividers (exact_div.h)
  void SetBand(uint32_t row_begin_, uint32_t stripe_rows_, uint32_t stripe_period_) {    // the fields and their dividers together (as RenderArgs::SetBand; call once `scene` is set)
    row_begin = row_begin_; stripe_rows = stripe_rows_; stripe_period = stripe_period_;
    div_stripe_rows = MakeExactDiv(stripe_rows_); div_width = MakeExactDiv(scene.sensor.w);
  }
};

template <int kEngine>
__global__ void __launch_bounds__(256, kEngine == ENGINE_BVH ? AMBER_QUERY_WAVES : 1) aov_kernel(const AovArgs a) {
  const DevScene& sc = a.scene;
  const EngineLds lds = StageEngineLds<kEngine, AMBER_BVH_STACK>(sc);
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * 256u; base < a.n_pixels; base += static_cast<uint64_t>(gridDim.x) * 256u) {   // uniform over the workgroup
    const uint64_t i = base + threadIdx.x;
    const bool mine = i < a.n_pixels;
    const PathPlace at = PlacePixel(a, static_cast<uint32_t>(ClampToLastItem<uint64_t>(i, a.n_pixels)));
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
    if (mine) { s0 = a.aov[2u * i]; s1 = a.aov[2u * i + 1u]; }
    for (uint32_t k = 0; k < a.n_samples; ++k) {
      uint64_t rng = PathSeed(a, at, k);                // as the render kernels seed it
      V3 o, d; float ew; int origin_slot;
      GenerateEyeRay(sc, at.px, at.py, rng, o, d, ew, origin_slot);
      HitRec h;
      if constexpr (kEngine == ENGINE_BVH) {
        ClosestHitBvh<true>(sc, lds.stack, o, d, h);
      } else {
#ifdef AMBER_STAMPS
        StampCtx stamp_store{}; StampCtx* stamp_ctx = &stamp_store;
#endif
        ClosestHit<kEngine>(sc, lds.objects, lds.stack, o, d, origin_slot, h AMBER_STAMP_ARG);
      }
      if (h.idx >= 0 && !IsNanRay(o, d)) {
        V3 pos, nrm; uint32_t mat;
        ResolveHit<kEngine>(sc, lds.objects, h, o, d, pos, nrm, mat);
        const float* rho = sc.materials[mat].rho;
        s0.x = s0.x + rho[0]; s0.y = s0.y + rho[1]; s0.z = s0.z + rho[2]; s0.w = s0.w + h.t;
        s1.x = s1.x + nrm.x; s1.y = s1.y + nrm.y; s1.z = s1.z + nrm.z; s1.w = s1.w + 1.0f;
      }
    }
    if (mine) { a.aov[2u * i] = s0; a.aov[2u * i + 1u] = s1; }
  }
}

static_assert(sizeof(AmberAovPixel) == 32, "an AOV pixel is two float4");

// The AOV buffer of the band, zeroed by the first of the four entry points (and of the filters) that needs it: image_stage.inc's BandBuf
BandBuf AovBuf(amber_hip_pt* h) { return {{&h->img.aov}, 1, 2u, "AOV buffer"}; }
int EnsureAov(amber_hip_pt* h, const char* name) { return EnsureBand(h, AovBuf(h), name); }

int AovPass(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples) {
  const char* name = "amber_hip_pt_aov_pass";
  if (!h) return Fail(AMBER_EINVAL, std::string(name) + ": null handle");
  if (n_samples == 0) return AMBER_OK;
  if (static_cast<uint64_t>(first_sample) + n_samples > 0xffffffffull) return Fail(AMBER_EINVAL, std::string(name) + ": sample index overflow");
#if AMBER_BVH_WIDE
  return Fail(AMBER_EINVAL, std::string(name) + ": not part of an AMBER_BVH_WIDE measurement build");
#endif
  HIP_TRY(hipSetDevice(h->device));
  const uint32_t n_pixels = static_cast<uint32_t>(BandPixels(h));
  if (n_pixels == 0) return AMBER_OK;                                         // empty band
  AMBER_TRY(EnsureAov(h, name));
  AovArgs a{};
  a.scene = h->scene; a.aov = h->img.aov; a.hashed_seed = h->hashed_seed;
  a.n_pixels = n_pixels; a.first_sample = first_sample; a.n_samples = n_samples;
  a.SetBand(h->row_begin, h->stripe_rows, h->stripe_period);
  return LaunchPerItem(h, n_pixels, [&](auto engine, uint32_t n_blocks) {
    hipLaunchKernelGGL((aov_kernel<decltype(engine)::value>), dim3(n_blocks), dim3(256), 0, h->stream, a);
  });
}

int AovClear(amber_hip_pt* h) { return BandClear(h, AovBuf, "amber_hip_pt_aov_clear"); }
int AovDownload(amber_hip_pt* h, AmberAovPixel* out) { return BandDownload(h, AovBuf, out, "amber_hip_pt_aov_download"); }
int DeviceAov(amber_hip_pt* h, void** dptr, uint64_t* n_pixels) { return BandPointer(h, AovBuf, dptr, n_pixels, "amber_hip_pt_device_aov"); }

}  // namespace

// resolve.inc -- amber_hip_pt_resolve: the framebuffer's sums turned into what a display or an encoder accepts, on the device: the mean
// (sum / n_samples), and postprocess::Filmic + postprocess::Gamma(2.2) down to 8 bits (filmic.cc:30-66, gamma.cc:36-52; the host's restatement
// is amber/postprocess.cc, the oracle's oracle_tonemap).  Part of the one translation unit pt_host.hip; Pow is the render kernels' (dev_math.h).
//
//   resolve_kernel<kFormat, kMirror>   a streaming kernel sized by bytes: one thread per FOUR consecutive output pixels -- three 16-byte loads of
//                                      the sums (48 bytes) and, per format, three 16-byte stores (MEAN_F32), three 32-bit stores (RGB8) or one
//                                      16-byte store (RGBA8); no byte stores on that path.  Under AMBER_RESOLVE_MIRROR_X the four output pixels
//                                      are four input pixels of the same row in reverse order; their 48 bytes start on a 4-byte boundary only
//                                      (still three 16-byte loads: global memory takes them at dword alignment).  A group that is not four whole
//                                      pixels of one row -- the last n_pixels % 4 pixels, a mirrored group across a row end when width % 4 != 0,
//                                      every group when the caller's pointer is not 16-byte aligned -- goes pixel by pixel (per-group test).
// Arithmetic: every operation binary32 and rounded alone (-ffp-contract=off), in the order of oracle_tonemap; the constant products, kE / kF,
// Map(kW) and 1 / 2.2f are binary32 constant expressions there and here.  min is the comparison (p < 1) ? p : 1 -- std::min<float>(1, p) -- so a NaN
// p gives 1.  No LDS, no scratch, no tuning surface: 256 threads per workgroup, registers left to the compiler (twelve independent Pow per thread).
// Host side: the checks of the output arguments and the output tail (staging, launch, copy) are image_stage.inc's CheckBandOutput and WriteBandOutput,
// which the three filters share; this file holds the kernel, its launch and the entry point.
namespace {

constexpr float kFilmicA = 0.22f, kFilmicB = 0.30f, kFilmicC = 0.10f, kFilmicD = 0.20f, kFilmicE = 0.01f, kFilmicF = 0.30f, kFilmicW = 0.70f, kFilmicExposure = 16.0f;
constexpr float kFilmicBC = kFilmicB * kFilmicC, kFilmicDE = kFilmicD * kFilmicE, kFilmicDF = kFilmicD * kFilmicF, kFilmicEF = kFilmicE / kFilmicF;

__host__ __device__ constexpr float FilmicMap(float h) {                      // Filmic::Map, filmic.cc:59-66
  return (h * (h * kFilmicA + kFilmicBC) + kFilmicDE) / (h * (h * kFilmicA + kFilmicB) + kFilmicDF) - kFilmicEF;
}
constexpr float kFilmicWhite = FilmicMap(kFilmicW);
constexpr float kInvGamma = 1 / 2.2f;

__device__ __forceinline__ uint32_t ResolveByte(float mean) {
  const float mapped = FilmicMap(mean * kFilmicExposure) / kFilmicWhite;      // filmic.cc:52
  const float p = Pow(mapped, kInvGamma);
  const float v = 255 * ((p < 1.0f) ? p : 1.0f);                              // std::min<float>(1, p): 1 for a NaN p
  return v >= 0 ? static_cast<uint32_t>(v) : 0u;                              // truncation; v is in [0, 255]
}

struct alignas(4) Float4Dword { float x, y, z, w; };                          // 16 bytes at dword alignment (the mirrored loads)

template <int kFormat>
__device__ __forceinline__ void ResolveStorePixel(void* __restrict__ out, uint64_t p, float r, float g, float b) {
  if constexpr (kFormat == AMBER_RESOLVE_MEAN_F32) {
    float* o = static_cast<float*>(out) + 3u * p;
    o[0] = r; o[1] = g; o[2] = b;
  } else if constexpr (kFormat == AMBER_RESOLVE_RGB8) {
    uint8_t* o = static_cast<uint8_t*>(out) + 3u * p;
    o[0] = static_cast<uint8_t>(ResolveByte(r)); o[1] = static_cast<uint8_t>(ResolveByte(g)); o[2] = static_cast<uint8_t>(ResolveByte(b));
  } else {
    static_cast<uint32_t*>(out)[p] = ResolveByte(r) | ResolveByte(g) << 8 | ResolveByte(b) << 16 | 0xff000000u;
  }
}

// n_pixels < 2^32 (create refuses a larger sensor), so rows and columns are 32-bit divisions; element and byte offsets are 64-bit.
// n_vector: the pixels [0, n_vector) may go four at a time (a multiple of 4; 0 when the output pointer is not 16-byte aligned).
template <int kFormat, bool kMirror>
__global__ void __launch_bounds__(256) resolve_kernel(const float* __restrict__ fb, void* __restrict__ out, uint64_t n_pixels, uint64_t n_vector, uint32_t width, float n) {
  const uint64_t group = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
  const uint64_t p0 = group * 4u;                                             // first output pixel of the group
  if (p0 >= n_pixels) return;
  bool whole = p0 + 4u <= n_vector;
  uint64_t q0 = p0;                                                           // first (lowest) input pixel of a whole group
  if constexpr (kMirror) {
    const uint32_t y = static_cast<uint32_t>(p0) / width, x0 = static_cast<uint32_t>(p0) - y * width;
    whole = whole && x0 + 4u <= width;                                        // all four in row y
    q0 = static_cast<uint64_t>(y) * width + (width - 4u - x0);                // (only used when whole)
  }
  if (whole) {
    using Vec = typename std::conditional<kMirror, Float4Dword, float4>::type;
    const Vec* src = reinterpret_cast<const Vec*>(fb + 3u * q0);
    const Vec a = src[0], b = src[1], c = src[2];
    const float f[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
    float m[12];
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
      for (int ch = 0; ch < 3; ch++) m[3 * k + ch] = f[3 * (kMirror ? 3 - k : k) + ch] / n;
    if constexpr (kFormat == AMBER_RESOLVE_MEAN_F32) {
      float4* o = static_cast<float4*>(out) + 3u * group;
      o[0] = make_float4(m[0], m[1], m[2], m[3]); o[1] = make_float4(m[4], m[5], m[6], m[7]); o[2] = make_float4(m[8], m[9], m[10], m[11]);
    } else {
      uint32_t q[12];
#pragma unroll
      for (int i = 0; i < 12; i++) q[i] = ResolveByte(m[i]);
      if constexpr (kFormat == AMBER_RESOLVE_RGB8) {
        uint32_t* o = static_cast<uint32_t*>(out) + 3u * group;
        o[0] = q[0] | q[1] << 8 | q[2] << 16 | q[3] << 24;
        o[1] = q[4] | q[5] << 8 | q[6] << 16 | q[7] << 24;
        o[2] = q[8] | q[9] << 8 | q[10] << 16 | q[11] << 24;
      } else {
        static_cast<uint4*>(out)[group] = make_uint4(q[0] | q[1] << 8 | q[2] << 16 | 0xff000000u, q[3] | q[4] << 8 | q[5] << 16 | 0xff000000u,
                                                     q[6] | q[7] << 8 | q[8] << 16 | 0xff000000u, q[9] | q[10] << 8 | q[11] << 16 | 0xff000000u);
      }
    }
    return;
  }
  // the tail, a mirrored group across a row end, an output pointer without 16-byte alignment: pixel by pixel
#pragma unroll 1
  for (uint32_t k = 0; k < 4u; k++) {
    const uint64_t p = p0 + k;
    if (p >= n_pixels) break;
    uint64_t q = p;
    if constexpr (kMirror) {
      const uint32_t y = static_cast<uint32_t>(p) / width, x = static_cast<uint32_t>(p) - y * width;
      q = static_cast<uint64_t>(y) * width + (width - 1u - x);
    }
    const float* s = fb + 3u * q;
    ResolveStorePixel<kFormat>(out, p, s[0] / n, s[1] / n, s[2] / n);
  }
}

template <int kFormat>
void LaunchResolve(amber_hip_pt* h, const float* src, bool mirror, void* d_out, uint64_t n_pixels, float n) {   // WriteBandOutput's launch (image_stage.inc)
  const uint64_t n_vector = reinterpret_cast<uintptr_t>(d_out) % 16u == 0u ? n_pixels / 4u * 4u : 0u;
  const uint32_t n_blocks = static_cast<uint32_t>(((n_pixels + 3u) / 4u + 255u) / 256u);      // n_pixels < 2^32: at most 2^22 workgroups
  if (mirror) hipLaunchKernelGGL((resolve_kernel<kFormat, true>), dim3(n_blocks), dim3(256), 0, h->stream, src, d_out, n_pixels, n_vector, h->scene.sensor.w, n);
  else hipLaunchKernelGGL((resolve_kernel<kFormat, false>), dim3(n_blocks), dim3(256), 0, h->stream, src, d_out, n_pixels, n_vector, h->scene.sensor.w, n);
}

int Resolve(amber_hip_pt* h, uint32_t n_samples, uint32_t format, void* out, uint64_t out_bytes, uint32_t flags) {
  const std::string name = "amber_hip_pt_resolve";
  if (!h) return Fail(AMBER_EINVAL, name + ": null handle");
  if (n_samples == 0) return Fail(AMBER_EINVAL, name + ": n_samples is 0");
  BandOutput o{};
  { const int rc = CheckBandOutput(h, name, false, format, out, out_bytes, flags, o); if (rc != AMBER_OK || o.n_pixels == 0) return rc; }
  HIP_TRY(hipSetDevice(h->device));
  // a pass whose record buffer was sized from an estimate may have to be repeated before its sums stand (SettlePending): wait for that one, as
  // clear and download do; a pass with a slot for every path, and every pass of the item kernel, needs no waiting
  AMBER_TRY(SettlePending(h));
  return WriteBandOutput(h, o, format, h->d_fb, static_cast<float>(n_samples), out);
}

}  // namespace

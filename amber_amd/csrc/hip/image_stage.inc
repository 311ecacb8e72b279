// image_stage.inc -- what the files of the image stage share: everything that runs on the band after accumulation (resolve.inc, aov.inc, denoise.inc,
// denoise_variance.inc, temporal.inc; the stage's buffers are the handle's ImageStageBufs, pt_host.hip).  Part of the one translation unit pt_host.hip.
//   BandPixels          the band's pixel count (pt_host.hip and lab_api.inc use it too)
//   BandBuf             a buffer, or several that stand or fall together, of float4 records per band pixel, allocated and zeroed by the first call that
//                       needs it: EnsureBand, BandClear, BandDownload, BandPointer.  The AOV sums, the moments and the history are such buffers.
//   CheckBandOutput     what the output arguments of amber_hip_pt_resolve and of the three filters must satisfy, in one order
//   WriteBandOutput     the output tail of those four: resolve.inc's kernel from the summed or filtered source into the caller's pointer or the staging
//                       buffer, and for AMBER_RESOLVE_HOST the copy and the wait
//   CheckFilterParams   what the three filters' params structs share
//   device helpers     the squared distance, clamp0, the three guide stops, the luminance and the guide record {a.xyz, z} {n.xyz, rz} of the filters' kernels
namespace {

uint64_t BandPixels(const amber_hip_pt* h) { return static_cast<uint64_t>(h->local_rows) * h->scene.sensor.w; }

// ---- device helpers of the filters' kernels: each a fixed sequence of binary32 operations, rounded alone
__device__ __forceinline__ float DenoiseSq(float u0, float u1, float u2, float v0, float v1, float v2) {
  const float d0 = u0 - v0, d1 = u1 - v1, d2 = u2 - v2;
  return (d0 * d0 + d1 * d1) + d2 * d2;
}
__device__ __forceinline__ float DenoiseClamp0(float t) { return t > 0.f ? t : 0.f; }     // 0 for a NaN t
// (tn * ta) * tz: the three guide stops of a tap q seen from p, guide records {a.xyz, z} {n.xyz, rz}
__device__ __forceinline__ float DenoiseGuideStop(const float4& pa, const float4& pn, const float4& qa, const float4& qn, float k_normal, float k_albedo, float k_depth) {
  const float tn = DenoiseClamp0(1.0f - DenoiseSq(pn.x, pn.y, pn.z, qn.x, qn.y, qn.z) * k_normal);
  const float ta = DenoiseClamp0(1.0f - DenoiseSq(pa.x, pa.y, pa.z, qa.x, qa.y, qa.z) * k_albedo);
  const float tz = DenoiseClamp0(1.0f - (fabsf(pa.w - qa.w) * pn.w) * k_depth);
  return (tn * ta) * tz;
}
__device__ __forceinline__ float DvLuminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
// The guide record of a pixel from its AOV sums {albedo.rgb, depth} {normal.xyz, coverage}: the divisions by coverage and the reciprocal of the depth,
// done once per pixel, not once per tap; zeros without coverage
__device__ __forceinline__ void GuideRecord(const float4& a0, const float4& a1, float4& g0, float4& g1) {
  const float cov = a1.w;
  g0 = make_float4(0.f, 0.f, 0.f, 0.f); g1 = g0;
  if (cov > 0.f) {
    g0.x = a0.x / cov; g0.y = a0.y / cov; g0.z = a0.z / cov; g0.w = a0.w / cov;
    g1.x = a1.x / cov; g1.y = a1.y / cov; g1.z = a1.z / cov;
  }
  g1.w = g0.w > 0.f ? 1.0f / g0.w : 0.f;
}

// ---- band buffers
struct BandBuf {
  DevBuf<float4>* buf[4]; int n;                  // allocated together or not at all; buf[0] is the one that clear, download and pointer mean
  uint32_t vecs;                                  // float4s per band pixel
  const char* what;                               // hipMalloc(<what>)
};
using BandBufOf = BandBuf (*)(amber_hip_pt*);     // the buffer of a handle that is not null

// Allocated and zeroed (on the handle's stream) by the first call that needs the buffer; nothing for an empty band.
int EnsureBand(amber_hip_pt* h, const BandBuf& b, const char* name) {
  const size_t n_vecs = static_cast<size_t>(BandPixels(h)) * b.vecs;
  if (n_vecs == 0 || *b.buf[0]) return AMBER_OK;
  DevBuf<float4> fresh[4];
  for (int i = 0; i < b.n; i++) {
    const hipError_t e = fresh[i].alloc(n_vecs);
    if (e != hipSuccess) return Fail(AMBER_ENOMEM, std::string(name) + ": hipMalloc(" + b.what + "): " + hipGetErrorString(e));
    HIP_TRY(hipMemsetAsync(fresh[i], 0, n_vecs * sizeof(float4), h->stream));
  }
  for (int i = 0; i < b.n; i++) b.buf[i]->swap(fresh[i]);
  return AMBER_OK;
}

int BandClear(amber_hip_pt* h, BandBufOf of, const char* name) {
  if (!h) return Fail(AMBER_EINVAL, std::string(name) + ": null handle");
  HIP_TRY(hipSetDevice(h->device));
  const BandBuf b = of(h);
  const bool fresh = !*b.buf[0];                  // (zeroed by EnsureBand: no second fill)
  AMBER_TRY(EnsureBand(h, b, name));
  if (!fresh) HIP_TRY(hipMemsetAsync(*b.buf[0], 0, static_cast<size_t>(BandPixels(h)) * b.vecs * sizeof(float4), h->stream));
  return AMBER_OK;
}

int BandDownload(amber_hip_pt* h, BandBufOf of, void* out, const char* name) {
  if (!h || !out) return Fail(AMBER_EINVAL, std::string(name) + ": null handle or output pointer");
  HIP_TRY(hipSetDevice(h->device));
  const BandBuf b = of(h);
  AMBER_TRY(EnsureBand(h, b, name));
  const size_t bytes = static_cast<size_t>(BandPixels(h)) * b.vecs * sizeof(float4);
  if (bytes) HIP_TRY(hipMemcpyAsync(out, *b.buf[0], bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return AMBER_OK;
}

int BandPointer(amber_hip_pt* h, BandBufOf of, void** dptr, uint64_t* n_pixels, const char* name) {
  if (!h || !dptr) return Fail(AMBER_EINVAL, std::string(name) + ": null handle or pointer");
  HIP_TRY(hipSetDevice(h->device));
  const BandBuf b = of(h);
  AMBER_TRY(EnsureBand(h, b, name));
  *dptr = b.buf[0]->p;                                                        // (null for an empty band)
  if (n_pixels) *n_pixels = BandPixels(h);
  return AMBER_OK;
}

// ---- output
constexpr uint64_t kResolveBytesPerPixel[3] = {12u, 3u, 4u};                  // MEAN_F32, RGB8, RGBA8

// What the output arguments must satisfy, checked in this order, and what the launches need of them.  `filter`: the three filters, which refuse a
// striped handle and launch tiles of 64 x 4 pixels; amber_hip_pt_resolve does neither.  AMBER_OK with n_pixels == 0: an empty band, nothing to do.
struct BandOutput { uint32_t width, rows, blocks_x; uint64_t n_pixels, want, n_tiles; bool host, mirror; };

int CheckBandOutput(const amber_hip_pt* h, const std::string& name, bool filter, uint32_t format, const void* out, uint64_t out_bytes, uint32_t flags, BandOutput& o) {
  o = BandOutput{};
  if (format > AMBER_RESOLVE_RGBA8) return Fail(AMBER_EINVAL, name + ": unknown format " + std::to_string(format));
  if (flags & ~static_cast<uint32_t>(AMBER_RESOLVE_HOST | AMBER_RESOLVE_MIRROR_X)) return Fail(AMBER_EINVAL, name + ": unknown flag bits");
  if (filter && h->stripe_period != 0u) return Fail(AMBER_EINVAL, name + ": a striped handle's local rows are not neighbours in the frame; filter a contiguous band");
  const uint32_t width = h->scene.sensor.w, rows = h->local_rows;
  const uint64_t n_pixels = BandPixels(h);
  const uint64_t want = n_pixels * kResolveBytesPerPixel[format];
  if (out_bytes != want)
    return Fail(AMBER_EINVAL, name + ": out_bytes is " + std::to_string(out_bytes) + ", the band takes exactly " + std::to_string(want) + " (" + std::to_string(rows) +
                                  " rows of " + std::to_string(width) + " pixels, " + std::to_string(kResolveBytesPerPixel[format]) + " bytes each)");
  if (n_pixels == 0) return AMBER_OK;                                         // empty band
  if (!out) return Fail(AMBER_EINVAL, name + ": null output pointer");
  const bool host = (flags & AMBER_RESOLVE_HOST) != 0u;
  if (!host && format != AMBER_RESOLVE_RGB8 && reinterpret_cast<uintptr_t>(out) % 4u != 0u)
    return Fail(AMBER_EINVAL, name + ": a device pointer for MEAN_F32 or RGBA8 must be 4-byte aligned");
  const uint32_t blocks_x = (width + 63u) / 64u;
  const uint64_t n_tiles = static_cast<uint64_t>(blocks_x) * ((rows + 3u) / 4u);
  if (filter && n_tiles > 0x7fffffffull) return Fail(AMBER_EINVAL, name + ": band too large for one launch");
  o.width = width; o.rows = rows; o.blocks_x = blocks_x; o.n_pixels = n_pixels; o.want = want; o.n_tiles = n_tiles;
  o.host = host; o.mirror = (flags & AMBER_RESOLVE_MIRROR_X) != 0u;
  return AMBER_OK;
}

template <int kFormat>
void LaunchResolve(amber_hip_pt* h, const float* src, bool mirror, void* d_out, uint64_t n_pixels, float n);    // resolve.inc

// src: sums of the band's layout and their sample count (the framebuffer; a filtered mean with n = 1: x / 1.0f == x).  AMBER_RESOLVE_HOST stages
// through a buffer of the handle, grown on first use and reused.
int WriteBandOutput(amber_hip_pt* h, const BandOutput& o, uint32_t format, const float* src, float n, void* out) {
  void* d_out = out;
  if (o.host) {
    AMBER_TRY(Grow(h, h->img.resolve_out, o.want, "resolve staging"));
    d_out = h->img.resolve_out.p;
  }
  if (format == AMBER_RESOLVE_MEAN_F32) LaunchResolve<AMBER_RESOLVE_MEAN_F32>(h, src, o.mirror, d_out, o.n_pixels, n);
  else if (format == AMBER_RESOLVE_RGB8) LaunchResolve<AMBER_RESOLVE_RGB8>(h, src, o.mirror, d_out, o.n_pixels, n);
  else LaunchResolve<AMBER_RESOLVE_RGBA8>(h, src, o.mirror, d_out, o.n_pixels, n);
  HIP_TRY(hipGetLastError());
  if (o.host) {
    HIP_TRY(hipMemcpyAsync(out, d_out, o.want, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  return AMBER_OK;
}

// ---- the filters' parameters
// A params struct P has levels, k_normal, k_albedo, k_depth, a fourth constant, reserved words and at most one more field with a range of its own,
// which is checked where it stands in P: in front of the constants or behind them.
template <typename P>
struct FilterExtra { uint32_t P::*field; const char* field_name; uint32_t lo, hi; bool before_k; };

template <typename P>
int CheckFilterParams(const std::string& name, const amber_hip_pt* h, const P* params, uint32_t n_samples, uint32_t min_levels, float P::*k4, const char* k4_name,
                      const FilterExtra<P>* extra = nullptr) {
  if (!h) return Fail(AMBER_EINVAL, name + ": null handle");
  if (!params) return Fail(AMBER_EINVAL, name + ": null params");
  if (n_samples == 0) return Fail(AMBER_EINVAL, name + ": n_samples is 0");
  auto in_range = [&](const char* field_name, uint32_t v, uint32_t lo, uint32_t hi) -> int {
    if (v >= lo && v <= hi) return AMBER_OK;
    return Fail(AMBER_EINVAL, name + ": " + field_name + " is " + std::to_string(v) + ", not " + std::to_string(lo) + " .. " + std::to_string(hi));
  };
  AMBER_TRY(in_range("levels", params->levels, min_levels, 8u));
  if (extra && extra->before_k) AMBER_TRY(in_range(extra->field_name, params->*extra->field, extra->lo, extra->hi));
  const float k[4] = {params->k_normal, params->k_albedo, params->k_depth, params->*k4};
  const char* k_name[4] = {"k_normal", "k_albedo", "k_depth", k4_name};
  for (int i = 0; i < 4; i++)
    if (!(k[i] >= 0.f) || std::isinf(k[i])) return Fail(AMBER_EINVAL, name + ": " + k_name[i] + " is negative, NaN or infinite");
  if (extra && !extra->before_k) AMBER_TRY(in_range(extra->field_name, params->*extra->field, extra->lo, extra->hi));
  uint32_t reserved = 0u;
  for (const uint32_t r : params->reserved) reserved |= r;
  if (reserved) return Fail(AMBER_EINVAL, name + ": reserved fields must be 0");
  return AMBER_OK;
}

}  // namespace

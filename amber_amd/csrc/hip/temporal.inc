// temporal.inc -- amber_hip_pt_temporal / _temporal_reset / _history_download / amber_hip_pt_device_history: a per-pixel history of the band's mean
// image, carried from frame to frame.  The previous frames' colour is reprojected through the previous lens (the chief ray: the same for the pinhole
// and the thin lens), validated against the previous frame's guide record with amber_hip_pt_denoise's three guide stops, blended with this frame's
// mean as a running mean of capped length, and handed to denoise.inc's level kernel and resolve.inc's output stage.  A fixed sequence of binary32
// operations, each rounded alone (-ffp-contract=off); the contract of include/amber_hip.h states it (its numpy restatement: tests/temporal_reference.py).
// Part of the one translation unit pt_host.hip; the guide record, DenoiseGuideStop, lum, the history's BandBuf, the checks of the parameters and of the
// output arguments and the output tail are image_stage.inc's, the levels denoise.inc's LaunchDenoiseLevels.
//
//   temporal_kernel   ONE kernel for prepare, reprojection, validation, blend and the three writes (no denoise_prepare_kernel in front of it): one
//                     thread per band pixel on the level kernel's 64 x 4 tile, so a wave is 64 consecutive pixels of a row.  Per pixel it reads this
//                     frame's 12 + 32 bytes, gathers up to four previous history records and four previous guide records (two float4 each) and writes
//                     the new history record (32 bytes), this frame's guide record (32 bytes: the level kernel's guide and the next frame's previous
//                     guide are the same buffer) and the accumulated colour (12 bytes, what the level kernel and resolve's kernel read).  Under a
//                     camera move neighbouring lanes land on neighbouring previous pixels: the gather is near-coalesced and the 2 x 2 footprints
//                     overlap in cache.  The taps are branch-free, as denoise_level_kernel's are and for its reason: a tap that is not taken loads the
//                     pixel's own record and adds +0, so the sixteen float4 loads of a pixel are in flight together.  The only branch is on `mode`,
//                     which is uniform over the launch.  Both lenses and the sensor constants travel by value in the kernel arguments.
// No LDS, no atomics, no scratch, no tuning surface: 256 threads per workgroup, registers left to the compiler.
// Buffers of the handle, allocated and zeroed by the first call that needs them (not by a reset): two history buffers and two guide buffers used ping-pong (a call reads
// pair `cur`, writes the other one and makes it `cur` once everything has been enqueued without an error), 2 x (32 + 32) bytes per band pixel.  The
// levels ping-pong through denoise.inc's two colour buffers.
namespace {

static_assert(sizeof(AmberTemporalParams) == 32, "AmberTemporalParams is 32 bytes");
static_assert(sizeof(AmberHistoryPixel) == 32, "a history pixel is two float4");

enum { TEMPORAL_EMPTY = 0, TEMPORAL_SAME_LENS = 1, TEMPORAL_MOVED_LENS = 2 };

struct TemporalLens { float origin[3]; float m[9]; float sensor_distance; };   // m: global_ of this call's lens, local_ of the previous call's

struct TemporalArgs {
  const float* fb;                                // the sums: 3 floats per band pixel
  const float4* aov;                              // the AOV sums: two float4 per band pixel
  const float4* hist_in;                          // previous history: {color.rgb, length} {m1, m2, 0, 0}
  const float4* guide_in;                         // previous guide: {a.xyz, z} {n.xyz, rz}
  float4* hist_out;
  float4* guide_out;
  float* color_out;                               // the accumulated colour, 3 floats per band pixel
  uint32_t width, rows, blocks_x, row_begin;      // the band; tiles of 64 pixels per tile row; the global row of local row 0
  uint32_t mode;                                  // TEMPORAL_*
  float n, max_history, k_normal, k_albedo, k_depth;
  float wf, hf, sw, sh;                           // DevSensor's
  TemporalLens now, before;
};

__global__ void __launch_bounds__(256) temporal_kernel(const TemporalArgs a) {
  const uint32_t by = blockIdx.x / a.blocks_x, bx = blockIdx.x - by * a.blocks_x;
  const uint32_t x = bx * 64u + (threadIdx.x & 63u), y = by * 4u + (threadIdx.x >> 6);
  if (x >= a.width || y >= a.rows) return;
  const uint64_t p = static_cast<uint64_t>(y) * a.width + x;
  // ---- this frame: denoise_prepare_kernel's mean and guide record, and the luminance
  const float* s = a.fb + 3u * p;
  const float cr = s[0] / a.n, cg = s[1] / a.n, cb = s[2] / a.n;
  const float4 a0 = a.aov[2u * p], a1 = a.aov[2u * p + 1u];
  const bool covered = a1.w > 0.f;
  float4 g0, g1;
  GuideRecord(a0, a1, g0, g1);
  const float yl = DvLuminance(cr, cg, cb);
  // ---- where the pixel was: the taps' local coordinates, their weights, the expected depth
  int64_t ix = static_cast<int64_t>(x), iy = static_cast<int64_t>(y);
  float b[4] = {1.0f, 0.f, 0.f, 0.f};
  float d = g0.w;
  bool usable = a.mode != TEMPORAL_EMPTY;
  const bool four = a.mode == TEMPORAL_MOVED_LENS;
  if (four) {
    const float uvx = (static_cast<float>(x) + 0.5f) / a.wf, uvy = (static_cast<float>(a.row_begin + y) + 0.5f) / a.hf;
    const V3 sensor_point = v3((uvx - 0.5f) * a.sw, (uvy - 0.5f) * a.sh, a.now.sensor_distance);
    const V3 dir = Normalize(MatMul(a.now.m, -sensor_point));                  // the plain form: __builtin_sqrtf, three divisions
    const V3 world = ld3(a.now.origin) + g0.w * dir;
    const V3 v = world - ld3(a.before.origin);
    const V3 dl = MatMul(a.before.m, v);
    const V3 pt = (a.before.sensor_distance / dl.z) * dl;
    const float fx = (pt.x / a.sw + 0.5f) * a.wf - 0.5f, fy = (pt.y / a.sh + 0.5f) * a.hf - 0.5f;
    d = __builtin_sqrtf(SquaredLength(v));
    const bool valid = dl.z < 0.f && fx > -1.0f && fx < a.wf && fy > -1.0f && fy < a.hf;      // false for a NaN
    usable = usable && valid && covered;
    const float flx = valid ? __builtin_floorf(fx) : 0.f, fly = valid ? __builtin_floorf(fy) : 0.f;
    const float ax = fx - flx, ay = fy - fly, ux = 1.0f - ax, uy = 1.0f - ay;
    b[0] = ux * uy; b[1] = ax * uy; b[2] = ux * ay; b[3] = ax * ay;
    ix = static_cast<int64_t>(flx); iy = static_cast<int64_t>(fly) - static_cast<int64_t>(a.row_begin);
  }
  float4 pa = g0, pn = g1;
  pa.w = d; pn.w = 1.0f / d;
  float sr = 0.f, sg = 0.f, sb = 0.f, sl = 0.f, s1 = 0.f, s2 = 0.f, bsum = 0.f;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int64_t qx = ix + (k & 1), qy = iy + (k >> 1);
    const bool inside = (k == 0 || four) && qx >= 0 && qx < static_cast<int64_t>(a.width) && qy >= 0 && qy < static_cast<int64_t>(a.rows);
    const uint64_t q = inside ? static_cast<uint64_t>(qy) * a.width + static_cast<uint64_t>(qx) : p;     // a tap not taken loads the pixel's own record and adds nothing
    const float4 h0 = a.hist_in[2u * q], h1 = a.hist_in[2u * q + 1u];
    const float4 qa = a.guide_in[2u * q], qn = a.guide_in[2u * q + 1u];
    const bool had = qn.w > 0.f;                                                // the previous guide there had coverage (a hit at a positive mean depth)
    const float stop = DenoiseGuideStop(pa, pn, qa, qn, a.k_normal, a.k_albedo, a.k_depth);
    const bool take = usable && inside && h0.w > 0.f && (covered ? (had && stop > 0.f) : !had);
    const float w = b[k];
    sr = sr + (take ? w * h0.x : 0.f); sg = sg + (take ? w * h0.y : 0.f); sb = sb + (take ? w * h0.z : 0.f); sl = sl + (take ? w * h0.w : 0.f);
    s1 = s1 + (take ? w * h1.x : 0.f); s2 = s2 + (take ? w * h1.y : 0.f); bsum = bsum + (take ? w : 0.f);
  }
  // ---- blend
  float4 o0 = make_float4(cr, cg, cb, 1.0f), o1 = make_float4(yl, yl * yl, 0.f, 0.f);
  if (bsum > 0.01f) {
    const float hr = sr / bsum, hg = sg / bsum, hb = sb / bsum, hl = sl / bsum, h1 = s1 / bsum, h2 = s2 / bsum;
    const float grown = hl + 1.0f;
    const float len = grown < a.max_history ? grown : a.max_history;
    const float alpha = 1.0f / len;
    o0 = make_float4(hr + (cr - hr) * alpha, hg + (cg - hg) * alpha, hb + (cb - hb) * alpha, len);
    o1 = make_float4(h1 + (yl - h1) * alpha, h2 + (yl * yl - h2) * alpha, 0.f, 0.f);
  }
  a.hist_out[2u * p] = o0; a.hist_out[2u * p + 1u] = o1;
  a.guide_out[2u * p] = g0; a.guide_out[2u * p + 1u] = g1;
  float* c = a.color_out + 3u * p;
  c[0] = o0.x; c[1] = o0.y; c[2] = o0.z;
}

// The words of AmberFlatThinLens a lens update may change, as the handle's DevLens keeps them (first_blade_object never changes)
bool TemporalSameLens(const DevLens& u, const DevLens& v) {
  return std::memcmp(u.origin, v.origin, sizeof u.origin) == 0 && std::memcmp(u.global_, v.global_, sizeof u.global_) == 0 &&
         std::memcmp(u.local_, v.local_, sizeof u.local_) == 0 && std::memcmp(&u.focus_distance, &v.focus_distance, 4) == 0 &&
         std::memcmp(&u.sensor_distance, &v.sensor_distance, 4) == 0 && std::memcmp(&u.p_area, &v.p_area, 4) == 0 && u.n_blades == v.n_blades && u.kind == v.kind;
}

// The two history buffers and the two guide buffers of the band, zeroed together by the first entry point that needs them: image_stage.inc's BandBuf,
// the current history in front (until there is one, pair 0 is current and the history empty)
BandBuf HistoryBuf(amber_hip_pt* h) {
  ImageStageBufs& img = h->img;
  return {{&img.history[img.history_cur], &img.history[img.history_cur ^ 1u], &img.history_guide[0], &img.history_guide[1]}, 4, 2u, "history buffers"};
}
int EnsureHistory(amber_hip_pt* h, const char* name) { return EnsureBand(h, HistoryBuf(h), name); }

int Temporal(amber_hip_pt* h, uint32_t n_samples, const AmberTemporalParams* params, uint32_t format, void* out, uint64_t out_bytes, uint32_t flags) {
  const std::string name = "amber_hip_pt_temporal";
  const FilterExtra<AmberTemporalParams> history{&AmberTemporalParams::max_history, "max_history", 1u, 65535u, true};
  AMBER_TRY(CheckFilterParams(name, h, params, n_samples, 0u, &AmberTemporalParams::k_color, "k_color", &history));
  BandOutput o{};
  { const int rc = CheckBandOutput(h, name, true, format, out, out_bytes, flags, o); if (rc != AMBER_OK || o.n_pixels == 0) return rc; }
  AMBER_TRY(BeginFilter(h, name));
  AMBER_TRY(EnsureHistory(h, name.c_str()));
  ImageStageBufs& img = h->img;
  for (DevBuf<float>& c : img.denoise_color) AMBER_TRY(Grow(h, c, static_cast<size_t>(o.n_pixels) * 3u, "denoise colour"));
  const uint32_t cur = img.history_cur, next = cur ^ 1u;
  TemporalArgs t{};
  t.fb = h->d_fb; t.aov = img.aov; t.hist_in = img.history[cur]; t.guide_in = img.history_guide[cur];
  t.hist_out = img.history[next]; t.guide_out = img.history_guide[next]; t.color_out = img.denoise_color[0];
  t.width = o.width; t.rows = o.rows; t.blocks_x = o.blocks_x; t.row_begin = h->row_begin;
  t.mode = img.history_empty ? TEMPORAL_EMPTY : TemporalSameLens(h->lens, img.history_lens) ? TEMPORAL_SAME_LENS : TEMPORAL_MOVED_LENS;
  t.n = static_cast<float>(n_samples); t.max_history = static_cast<float>(params->max_history);
  t.k_normal = params->k_normal; t.k_albedo = params->k_albedo; t.k_depth = params->k_depth;
  t.wf = h->scene.sensor.wf; t.hf = h->scene.sensor.hf; t.sw = h->scene.sensor.sw; t.sh = h->scene.sensor.sh;
  std::memcpy(t.now.origin, h->lens.origin, sizeof t.now.origin); std::memcpy(t.now.m, h->lens.global_, sizeof t.now.m); t.now.sensor_distance = h->lens.sensor_distance;
  if (t.mode == TEMPORAL_MOVED_LENS) {                                        // (the only mode that reads it)
    const DevLens& before = img.history_lens;
    std::memcpy(t.before.origin, before.origin, sizeof t.before.origin); std::memcpy(t.before.m, before.local_, sizeof t.before.m); t.before.sensor_distance = before.sensor_distance;
  }
  hipLaunchKernelGGL(temporal_kernel, dim3(static_cast<uint32_t>(o.n_tiles)), dim3(256), 0, h->stream, t);
  const float* filtered = LaunchDenoiseLevels(h, o, img.history_guide[next], params->levels, params->k_normal, params->k_albedo, params->k_depth, params->k_color);
  AMBER_TRY(WriteBandOutput(h, o, format, filtered, 1.0f, out));
  // the commit: until here the history in use is what it was (the kernel wrote the other pair)
  img.history_cur = next; img.history_lens = h->lens; img.history_empty = false;
  return AMBER_OK;
}

int TemporalReset(amber_hip_pt* h) {
  const char* name = "amber_hip_pt_temporal_reset";
  if (!h) return Fail(AMBER_EINVAL, std::string(name) + ": null handle");
  HIP_TRY(hipSetDevice(h->device));
  // a history never used is empty and reads as zeros already: nothing is allocated for it (an empty band never has one); an emptied one reads as zeros too
  DevBuf<float4>& current = h->img.history[h->img.history_cur];
  if (current) HIP_TRY(hipMemsetAsync(current, 0, static_cast<size_t>(BandPixels(h)) * sizeof(AmberHistoryPixel), h->stream));
  h->img.history_empty = true;
  return AMBER_OK;
}

// (the CURRENT history: the next amber_hip_pt_temporal moves it)
int HistoryDownload(amber_hip_pt* h, AmberHistoryPixel* out) { return BandDownload(h, HistoryBuf, out, "amber_hip_pt_history_download"); }
int DeviceHistory(amber_hip_pt* h, void** dptr, uint64_t* n_pixels) { return BandPointer(h, HistoryBuf, dptr, n_pixels, "amber_hip_pt_device_history"); }

}  // namespace

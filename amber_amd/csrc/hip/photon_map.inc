// photon_map.inc -- amber_hip_pm_build / amber_hip_pm_gather / amber_hip_pm_release: the handle's photon map and the k-nearest radiance gather.
// Part of the one translation unit pt_host.hip (kernels are launched from there); include/amber_hip.h states the contract, tests/photon_map_reference.py
// restates it in numpy.
//
// What the reference's photon family does with the list amber_hip_lt_trace_photons returns: PhotonMap::Search(point, radius, k), then
// sum(photon.Weight() * BSDF) * kernel() * weight (algorithm_sppm.cc:200-214).  The k-d tree is replaced by a uniform grid, which a device builds with
// one sort and searches without a stack:
//   build   1. bounds     per-axis minimum and maximum of the finite positions: a grid-stride reduction, per wave one atomicMin / atomicMax on the
//                         order-preserving bit pattern of the float; the host reads them back and fixes cell size and dimensions (the doubling rule)
//           2. keys       key = cell id, or `cells` for a dropped photon (one value past the grid: the sort moves them behind every kept photon)
//           3. sort       ONE stable rocprim::radix_sort_pairs of (key, input index) over the bits `cells` can set: within a cell, input order
//           4. starts     a thread per cell: lower bound of the cell id in the sorted keys (and the largest cell count, for the info record)
//           5. pack       {x, y, z, input index} (16 bytes: all the distance test reads) and {dir_out, 0} {weight, 0} (read for photons in radius only)
//   gather  a lane per query.  The cells the query's box touches are visited iz, iy, ix ascending; the cells of one (iz, iy) row are consecutive, so a row
//           is one run of the packed array.  One sweep counts the photons in radius and sums the first k of them: for N <= k that is the answer.
//           N > k (the slow path): T, the k-th smallest squared distance, by bisection over the BIT PATTERNS of d2 (d2 >= +0, so they order as unsigned
//           integers) -- every step is a counting sweep that also returns the nearest data values on both sides of the probe, so the interval snaps to
//           values that occur and the search ends as soon as a probe counts exactly k; then one sweep sums d2 < T and the first ties in visit order.
//           No per-lane heap: k = 1024 entries of (d2, index) per lane would be 512 KiB of scratch a wave, sifted through scattered memory, where the
//           sweeps re-read 16-byte records that the first sweep left in the caches (DESIGN.md, "Photon map").
// The sort is the handle's (IndexSortBufs: keys, permutations, rocPRIM's scratch), as for lt_accumulate.inc and lt_photons.inc.

namespace {

static_assert(sizeof(AmberGatherQuery) == 64 && sizeof(AmberGatherResult) == 32 && sizeof(AmberPhotonMapInfo) == 72, "a query is four float4, a result two");
static_assert(offsetof(AmberGatherQuery, radius) == 12 && offsetof(AmberGatherQuery, object) == 28 && offsetof(AmberGatherQuery, dir_out) == 32 && offsetof(AmberGatherQuery, weight) == 48, "the kernel's layout");
static_assert(offsetof(AmberGatherResult, n_used) == 12 && offsetof(AmberGatherResult, r2_used) == 16 && offsetof(AmberGatherResult, n_in_radius) == 20, "the kernel's layout");

constexpr uint64_t kPmMaxItems = 1ull << 31;      // photons of a build, queries of a gather, k
constexpr uint32_t kPmMaxDim = 1024u, kPmMaxCells = 1u << 22;
enum { PM_CTL_MIN = 0, PM_CTL_MAX = 3, PM_CTL_DROPPED = 6, PM_CTL_MAX_COUNT = 7, PM_CTL_WORDS = 8 };

// What the kernels need of the map, by value
struct PmGrid {
  const float4* __restrict__ posidx;
  const float4* __restrict__ payload;
  const uint32_t* __restrict__ start;
  float lo[3]; float inv;
  uint32_t dims[3]; uint32_t n_cells;
};

// float -> unsigned, order-preserving (-0 below +0); never called with NaN
__host__ __device__ __forceinline__ uint32_t PmOrdered(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
__host__ __device__ __forceinline__ uint32_t PmOrderedBack(uint32_t key) { return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key; }

__device__ __forceinline__ float PmCellF(float x, float lo, float inv) { return __builtin_floorf((x - lo) * inv); }
__device__ __forceinline__ bool PmFinite3(float4 p) { return IsFinite(p.x) && IsFinite(p.y) && IsFinite(p.z); }

__global__ void pm_init_kernel(uint32_t* __restrict__ ctl) {
  if (threadIdx.x < PM_CTL_WORDS) ctl[threadIdx.x] = threadIdx.x < PM_CTL_MAX ? 0xffffffffu : 0u;
}

__global__ void __launch_bounds__(256) pm_bounds_kernel(const float4* __restrict__ rec, uint64_t n, uint32_t* __restrict__ ctl) {
  uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u}, dropped = 0u;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += static_cast<uint64_t>(gridDim.x) * 256u) {
    const float4 p = rec[i * 4u];
    if (!PmFinite3(p)) { dropped++; continue; }
    const uint32_t o[3] = {PmOrdered(__float_as_uint(p.x)), PmOrdered(__float_as_uint(p.y)), PmOrdered(__float_as_uint(p.z))};
    for (int a = 0; a < 3; a++) { mn[a] = o[a] < mn[a] ? o[a] : mn[a]; mx[a] = o[a] > mx[a] ? o[a] : mx[a]; }
  }
  for (int off = 32; off > 0; off >>= 1) {
    for (int a = 0; a < 3; a++) {
      const uint32_t lo = __shfl_xor(mn[a], off), hi = __shfl_xor(mx[a], off);
      mn[a] = lo < mn[a] ? lo : mn[a]; mx[a] = hi > mx[a] ? hi : mx[a];
    }
    dropped += __shfl_xor(dropped, off);
  }
  if ((threadIdx.x & 63u) == 0u) {
    for (int a = 0; a < 3; a++) { atomicMin(&ctl[PM_CTL_MIN + a], mn[a]); atomicMax(&ctl[PM_CTL_MAX + a], mx[a]); }
    if (dropped) atomicAdd(&ctl[PM_CTL_DROPPED], dropped);
  }
}

// key = cell id (clamped to the grid: by construction it is inside), or n_cells for a dropped photon; index = identity
__global__ void __launch_bounds__(256) pm_key_kernel(const float4* __restrict__ rec, uint32_t n, const PmGrid g, unsigned long long* __restrict__ key, uint32_t* __restrict__ index) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float4 p = rec[static_cast<size_t>(i) * 4u];
  uint32_t cell = g.n_cells;
  if (PmFinite3(p)) {
    const float f[3] = {PmCellF(p.x, g.lo[0], g.inv), PmCellF(p.y, g.lo[1], g.inv), PmCellF(p.z, g.lo[2], g.inv)};
    uint32_t c[3];
    for (int a = 0; a < 3; a++) { const float top = static_cast<float>(g.dims[a] - 1u); c[a] = f[a] > 0.0f ? static_cast<uint32_t>(f[a] < top ? f[a] : top) : 0u; }
    cell = (c[2] * g.dims[1] + c[1]) * g.dims[0] + c[0];
  }
  key[i] = cell;
  index[i] = i;
}

__device__ __forceinline__ uint32_t PmLowerBound(const unsigned long long* __restrict__ key, uint32_t n, uint32_t value) {
  uint32_t lo = 0u, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (key[mid] < value) lo = mid + 1u; else hi = mid;
  }
  return lo;
}

// start[c] = the first of the n_kept sorted keys that is >= c, for c in [0, n_cells]; the largest cell count into ctl
__global__ void __launch_bounds__(256) pm_start_kernel(const unsigned long long* __restrict__ key, uint32_t n_kept, uint32_t n_cells, uint32_t* __restrict__ start, uint32_t* __restrict__ ctl) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  uint32_t count = 0u;
  if (c < n_cells) {
    const uint32_t s0 = PmLowerBound(key, n_kept, c), s1 = PmLowerBound(key, n_kept, c + 1u);
    start[c] = s0;
    if (c + 1u == n_cells) start[n_cells] = s1;
    count = s1 - s0;
  }
  for (int off = 32; off > 0; off >>= 1) { const uint32_t o = __shfl_xor(count, off); count = o > count ? o : count; }
  if ((threadIdx.x & 63u) == 0u && count) atomicMax(&ctl[PM_CTL_MAX_COUNT], count);
}

__global__ void __launch_bounds__(256) pm_pack_kernel(const float4* __restrict__ rec, const uint32_t* __restrict__ index, uint32_t n_kept, float4* __restrict__ posidx, float4* __restrict__ payload) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n_kept) return;
  const uint32_t i = index[j];
  const size_t r = static_cast<size_t>(i) * 4u;
  const float4 p = rec[r], d = rec[r + 1u], w = rec[r + 2u];                      // AmberPhoton: pos, object | dir_out, path | weight, sample | normal, bounce
  posidx[j] = make_float4(p.x, p.y, p.z, __uint_as_float(i));
  payload[static_cast<size_t>(j) * 2u] = make_float4(d.x, d.y, d.z, 0.f);
  payload[static_cast<size_t>(j) * 2u + 1u] = make_float4(w.x, w.y, w.z, 0.f);
}

// f(j, d2) for every photon of the cells [c0, c1] (per axis, inclusive) in visit order
template <typename F>
__device__ __forceinline__ void PmSweep(const PmGrid& g, const uint32_t (&c0)[3], const uint32_t (&c1)[3], V3 p, F&& f) {
  for (uint32_t iz = c0[2]; iz <= c1[2]; iz++) {
    for (uint32_t iy = c0[1]; iy <= c1[1]; iy++) {
      const uint32_t row = (iz * g.dims[1] + iy) * g.dims[0];
      const uint32_t end = g.start[row + c1[0] + 1u];
      for (uint32_t j = g.start[row + c0[0]]; j < end; j++) {
        const float4 q = g.posidx[j];
        const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
        f(j, (dx * dx + dy * dy) + dz * dz);
      }
    }
  }
}

__global__ void __launch_bounds__(256) pm_gather_kernel(const DevScene sc, const PmGrid g, uint32_t n, const float4* __restrict__ queries, float4* __restrict__ out, uint32_t k, uint32_t raw) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const size_t qi = static_cast<size_t>(i) * 4u, ri = static_cast<size_t>(i) * 2u;
  const float4 qa = queries[qi], qb = queries[qi + 1u], qc = queries[qi + 2u], qd = queries[qi + 3u];   // pos, radius | normal, object | dir_out, pad | weight, pad
  const V3 p = v3(qa.x, qa.y, qa.z), nrm = v3(qb.x, qb.y, qb.z), dir_out = v3(qc.x, qc.y, qc.z), weight = v3(qd.x, qd.y, qd.z);
  const float radius = qa.w;
  const int32_t object = __float_as_int(qb.w);
  if (!(PmFinite3(qa) && radius > 0.0f && IsFinite(radius) && object >= 0 && static_cast<uint32_t>(object) < sc.n_objects)) {
    out[ri] = make_float4(0.f, 0.f, 0.f, 0.f); out[ri + 1u] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const float r2 = radius * radius;
  // the cells the box [pos - radius, pos + radius] touches, cut to the grid as floats first (nothing huge is converted)
  uint32_t c0[3], c1[3];
  bool any = true;
  const float pp[3] = {p.x, p.y, p.z};
  for (int a = 0; a < 3; a++) {
    const float top = static_cast<float>(g.dims[a] - 1u);
    const float flo = PmCellF(pp[a] - radius, g.lo[a], g.inv), fhi = PmCellF(pp[a] + radius, g.lo[a], g.inv);
    if (fhi < 0.0f || flo > top) any = false;
    c0[a] = flo > 0.0f ? static_cast<uint32_t>(flo < top ? flo : top) : 0u;
    c1[a] = fhi < top ? static_cast<uint32_t>(fhi > 0.0f ? fhi : 0.0f) : g.dims[a] - 1u;
  }
  const DevMaterial m = sc.materials[sc.objects[object].material];
  const V3 rho = ld3(m.rho);
  V3 S = v3(0.f, 0.f, 0.f);
  auto add = [&](uint32_t j) {
    const float4 d = g.payload[static_cast<size_t>(j) * 2u], w = g.payload[static_cast<size_t>(j) * 2u + 1u];
    const float fs = SymmetricBSDF(m, nrm, dir_out, v3(d.x, d.y, d.z));
    S.x = S.x + w.x * (rho.x * fs); S.y = S.y + w.y * (rho.y * fs); S.z = S.z + w.z * (rho.z * fs);
  };
  uint32_t N = 0u;
  if (any) PmSweep(g, c0, c1, p, [&](uint32_t j, float d2) {
    if (d2 < r2) { if (k == 0u || N < k) add(j); N++; }
  });
  uint32_t n_used = N;
  float r2_used = r2;
  if (k != 0u && N > k) {
    // T = the k-th smallest d2.  Invariant: lo <= bits(T) <= hi, and count_hi = #{d2 <= hi}
    uint32_t lo = 0u, hi = __float_as_uint(r2) - 1u, count_hi = N;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      uint32_t count = 0u, below = 0u, above = 0xffffffffu;          // #{d2 <= mid}, the largest d2 <= mid, the smallest d2 > mid (in radius)
      PmSweep(g, c0, c1, p, [&](uint32_t, float d2) {
        if (d2 < r2) {
          const uint32_t u = __float_as_uint(d2);
          if (u <= mid) { count++; below = u > below ? u : below; } else { above = u < above ? u : above; }
        }
      });
      if (count >= k) { hi = below; count_hi = count; if (count == k) break; }
      else lo = above;
    }
    const float T = __uint_as_float(hi);
    uint32_t ties = 0xffffffffu;                                     // count_hi == k: every photon at distance T is used
    if (count_hi != k) {
      uint32_t nearer = 0u;
      PmSweep(g, c0, c1, p, [&](uint32_t, float d2) { if (d2 < T) nearer++; });
      ties = k - nearer;
    }
    S = v3(0.f, 0.f, 0.f);
    PmSweep(g, c0, c1, p, [&](uint32_t j, float d2) {
      if (d2 < T) add(j);
      else if (d2 == T && ties != 0u) { add(j); ties--; }
    });
    n_used = k; r2_used = T;
  }
  V3 rgb = S;
  if (!raw) {
    const float kern = 1.0f / ((3.14159274f * radius) * radius);      // DiskKernel (kernel.h:52): the query's radius, also when k shrank the search
    rgb = v3((S.x * kern) * weight.x, (S.y * kern) * weight.y, (S.z * kern) * weight.z);
  }
  out[ri] = make_float4(rgb.x, rgb.y, rgb.z, __uint_as_float(n_used));
  out[ri + 1u] = make_float4(r2_used, __uint_as_float(N), 0.f, 0.f);
}

PmGrid PmGridOf(const PhotonMapBufs& m, const AmberPhotonMapInfo& info) {
  PmGrid g{};
  g.posidx = m.posidx.p; g.payload = m.payload.p; g.start = m.start.p;
  for (int a = 0; a < 3; a++) { g.lo[a] = info.lo[a]; g.dims[a] = info.dims[a]; }
  g.inv = 1.0f / info.cell_size;
  g.n_cells = info.dims[0] * info.dims[1] * info.dims[2];
  return g;
}

int PmBuild(amber_hip_pt* h, const AmberPhoton* photons, uint64_t n, float cell_size, uint32_t flags, AmberPhotonMapInfo* out_info) {
  const std::string name = "amber_hip_pm_build";
  if (out_info) *out_info = AmberPhotonMapInfo{};
  if (!h) return Fail(AMBER_EINVAL, name + ": null handle");
  if (flags & ~static_cast<uint32_t>(AMBER_PHOTONS_HOST)) return Fail(AMBER_EINVAL, name + ": unknown flag bits");
  if (n > kPmMaxItems) return Fail(AMBER_EINVAL, name + ": more than 2^31 photons");
  if (!(cell_size > 0.0f) || !(cell_size < INFINITY)) return Fail(AMBER_EINVAL, name + ": cell_size must be positive and finite");
  if (n && !photons) return Fail(AMBER_EINVAL, name + ": null photons with a count");
  const bool host = (flags & AMBER_PHOTONS_HOST) != 0u;
  if (!host && (reinterpret_cast<uintptr_t>(photons) & 15u)) return Fail(AMBER_EINVAL, name + ": the device pointer must be 16-byte aligned");
  const auto t0 = std::chrono::steady_clock::now();
  HIP_TRY(hipSetDevice(h->device));
  PhotonMapBufs& m = h->pm;
  const hipStream_t st = h->stream;
  AmberPhotonMapInfo info{};
  info.n_photons = n; info.cell_size = cell_size;
  auto finish = [&]() -> int {                                          // the map stands
    info.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    m.info = info; m.built = true;
    if (out_info) *out_info = info;
    return AMBER_OK;
  };
  if (n == 0) { HIP_TRY(hipStreamSynchronize(st)); return finish(); }
  const float4* rec = reinterpret_cast<const float4*>(photons);
  if (host) {
    DevBuf<uint8_t>& staged = h->staging.in;                             // (HostStaging: the build reads it until the wait that ends this call)
    AMBER_TRY(Grow(h, staged, static_cast<size_t>(n) * sizeof(AmberPhoton), "photon map input"));
    HIP_TRY(hipMemcpyAsync(staged.p, photons, static_cast<size_t>(n) * sizeof(AmberPhoton), hipMemcpyHostToDevice, st));
    rec = reinterpret_cast<const float4*>(staged.p);
  }
  if (!m.ctl) HIP_TRY(m.ctl.alloc(PM_CTL_WORDS));
  AMBER_TRY(m.clock.Mark(0, st));
  // ---- 1. bounds, read back
  const uint32_t n32 = static_cast<uint32_t>(n);                        // (n <= 2^31)
  const dim3 wg(256), per_photon(static_cast<uint32_t>((n + 255u) / 256u));
  hipLaunchKernelGGL(pm_init_kernel, dim3(1), dim3(64), 0, st, m.ctl.p);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(pm_bounds_kernel, dim3(BlocksFor(n, static_cast<uint32_t>(h->n_cus) * 8u)), wg, 0, st, rec, n, m.ctl.p);
  HIP_TRY(hipGetLastError());
  uint32_t ctl[PM_CTL_WORDS] = {};
  HIP_TRY(hipMemcpyAsync(ctl, m.ctl.p, sizeof ctl, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  info.n_dropped = ctl[PM_CTL_DROPPED];
  const uint32_t n_kept = n32 - ctl[PM_CTL_DROPPED];
  if (n_kept == 0u) return finish();                                    // everything dropped: an empty map
  for (int a = 0; a < 3; a++) {
    const uint32_t lo = PmOrderedBack(ctl[PM_CTL_MIN + a]), hi = PmOrderedBack(ctl[PM_CTL_MAX + a]);
    std::memcpy(&info.lo[a], &lo, 4); std::memcpy(&info.hi[a], &hi, 4);
  }
  // ---- the doubling rule (binary32, every operation rounded alone: volatile keeps the host compiler from anything wider)
  volatile float c = cell_size;
  for (;;) {
    volatile float inv = 1.0f / c;
    bool ok = true;
    uint64_t cells = 1;
    for (int a = 0; a < 3 && ok; a++) {
      volatile float extent = info.hi[a] - info.lo[a];
      volatile float e = extent * inv;
      if (!(e < 2147483648.0f)) { ok = false; break; }
      info.dims[a] = static_cast<uint32_t>(std::floor(e)) + 1u;
      if (info.dims[a] > kPmMaxDim) ok = false;
      cells *= info.dims[a];
    }
    if (ok && cells <= kPmMaxCells) break;
    c = c * 2.0f;
    info.n_doublings++;
    if (!(c < INFINITY)) return Fail(AMBER_EINVAL, name + ": the extent of the photons overflows binary32: no cell size covers it");
  }
  info.cell_size = c;
  const uint32_t n_cells = info.dims[0] * info.dims[1] * info.dims[2];
  // ---- 2, 3. keys and the sort
  IndexSortBufs& sort = h->sort;
  AMBER_TRY(sort.Prepare(h, n32, BitsFor(n_cells + 1u), 0u, "photon map keys", "photon map order"));   // the dropped photons' key is n_cells
  m.built = false;                                                      // from here on the previous map is being replaced
  AMBER_TRY(Grow(h, m.start, static_cast<size_t>(n_cells) + 1u, "photon map cells"));
  AMBER_TRY(Grow(h, m.posidx, n_kept, "photon map positions"));
  AMBER_TRY(Grow(h, m.payload, static_cast<size_t>(n_kept) * 2u, "photon map payload"));
  const PmGrid g = PmGridOf(m, info);
  hipLaunchKernelGGL(pm_key_kernel, per_photon, wg, 0, st, rec, n32, g, sort.keys(), sort.order());
  HIP_TRY(hipGetLastError());
  AMBER_TRY(sort.Pass(0));
  // ---- 4, 5. cell starts, the packed arrays
  hipLaunchKernelGGL(pm_start_kernel, dim3((n_cells + 255u) / 256u), wg, 0, st, sort.sorted_keys(), n_kept, n_cells, m.start.p, m.ctl.p);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(pm_pack_kernel, dim3((n_kept + 255u) / 256u), wg, 0, st, rec, sort.order(), n_kept, m.posidx.p, m.payload.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(ctl, m.ctl.p, sizeof ctl, hipMemcpyDeviceToHost, st));
  AMBER_TRY(m.clock.Mark(1, st));
  HIP_TRY(hipStreamSynchronize(st));                                    // the caller's buffer is free, the cell statistics are here
  AMBER_TRY(m.clock.Lap(0, 1));
  info.max_cell_count = ctl[PM_CTL_MAX_COUNT];
  return finish();
}

// One launch over n queries in device memory (0 < n <= 2^31)
int LaunchPmGather(amber_hip_pt* h, uint64_t n, const float4* d_queries, float4* d_out, uint32_t k, bool raw) {
  PhotonMapBufs& m = h->pm;
  if (m.info.n_photons == m.info.n_dropped) {                            // the empty map answers zeros
    HIP_TRY(hipMemsetAsync(d_out, 0, static_cast<size_t>(n) * sizeof(AmberGatherResult), h->stream));
    return AMBER_OK;
  }
  hipLaunchKernelGGL(pm_gather_kernel, dim3(static_cast<uint32_t>((n + 255u) / 256u)), dim3(256), 0, h->stream, h->scene, PmGridOf(m, m.info), static_cast<uint32_t>(n),
                     d_queries, d_out, k, raw ? 1u : 0u);
  HIP_TRY(hipGetLastError());
  return AMBER_OK;
}

int PmGather(amber_hip_pt* h, uint64_t n, const AmberGatherQuery* q, AmberGatherResult* out, uint32_t k, uint32_t flags) {
  const std::string prefix = "amber_hip_pm_gather: ";
  AMBER_TRY(CheckQueryCall(h, prefix, flags, AMBER_RAYS_HOST | AMBER_PM_RAW_SUM, n, "queries"));
  if (k > kPmMaxItems) return Fail(AMBER_EINVAL, prefix + "k above 2^31");
  if (!h->pm.built) return Fail(AMBER_EINVAL, prefix + "the handle has no photon map (amber_hip_pm_build comes first; amber_hip_pm_release ends it)");
  if (n == 0) return AMBER_OK;
  AMBER_TRY(CheckQueryPointers(prefix, q, out, "queries"));
  const bool host = (flags & AMBER_RAYS_HOST) != 0u, raw = (flags & AMBER_PM_RAW_SUM) != 0u;
  if (!host && ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(out)) & 15u)) return Fail(AMBER_EINVAL, prefix + "device pointers must be 16-byte aligned");
  HIP_TRY(hipSetDevice(h->device));
  // one launch; the lab's clock brackets the launch alone (events 1, 2), not the copies of a trip
  auto launch = [&](uint64_t part, const void* d_q, void* d_out) -> int {
    StageClock<3>& clock = h->pm.clock;
    AMBER_TRY(clock.Mark(1, h->stream));
    AMBER_TRY(LaunchPmGather(h, part, static_cast<const float4*>(d_q), static_cast<float4*>(d_out), k, raw));
    AMBER_TRY(clock.Mark(2, h->stream));
    return clock.Lap(1, 2);
  };
  if (!host) return launch(n, q, out);
  return StagedTrips(h, n, kQueryStageRays, sizeof(AmberGatherQuery), sizeof(AmberGatherResult), q, out, "gather staging", launch);
}

// Gathers enqueued earlier may still read the map: the stream is waited for, then everything the map and its build own is released
int PmRelease(amber_hip_pt* h) {
  if (!h) return Fail(AMBER_EINVAL, "amber_hip_pm_release: null handle");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  PhotonMapBufs& m = h->pm;
  m.built = false; m.info = AmberPhotonMapInfo{};
  m.posidx.reset(); m.payload.reset(); m.start.reset(); m.ctl.reset();
  h->staging.in.reset(); h->staging.out.reset();                        // (the stream has been waited for: nobody holds them)
  return AMBER_OK;
}

}  // namespace

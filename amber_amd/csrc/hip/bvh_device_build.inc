// bvh_device_build.inc -- engine BVH's tree built on the device (AMBER_PT_FLAG_DEVICE_BUILD).  Part of the one translation unit pt_host.hip.
//
// Input: the DevObject array create has uploaded.  Output, in device memory owned by the handle, exactly what dev_bvh.h reads: bvh_nodes
// (DevBvhNodeQ), bvh_prims, bvh_objects, bvh_spheres, bvh_tris and the grid / margin scalars of DevScene.  The host builder (bvh_build.h) makes a
// binned-SAH tree in half a second for a million objects; this one makes a Morton-order radix tree in a few milliseconds.  The image does not
// depend on which: leaves are tested with the exact reference arithmetic and the (t, object index) rule, the tree only has to be CONSERVATIVE,
// and it is by the host builder's own formulae -- ObjectBox (sphere slack, needle reach), PadBox, F16AxisGrid, PlaneWordOutward are the
// functions of bvh_build.h compiled for the device, not restatements.
//
// Stages (one stream, in order; two host reads: 16 words after stage 5, nothing else):
//   1  db_bounds_raw      per-object geometric bounds -> scene bounds (the slack and the reach need the scene diagonal first, as in BuildBvh)
//   2  db_bounds_wide     widened bounds per object, centres; bounds of the widened boxes and of the centres
//   3  db_morton          63-bit Morton code of the centre over the centre bounds; rocPRIM radix sort of (code, object index) -- stable, so equal
//                         codes stay in index order and the order is a function of the scene alone
//   4  db_hierarchy       Karras 2012: inner node i of the radix tree over the top 24 bits of the sorted codes, then over the position (Delta)
//   5  db_boxes           bottom-up: a thread per sorted object walks towards the root; at every node the SECOND arrival continues with the union.
//                         Also the height of every node above the leaves (below).  db_live + an inclusive scan number the nodes that survive.
//   6  db_emit            a subtree of at most kLeafSize objects is ONE leaf (its objects are contiguous in the sorted order); the inner nodes above
//                         them are numbered by the scan in radix-tree order, so node 0 is the root; child boxes padded, quantised outward
//      db_gather          leaf-order object, sphere and triangle records (scene_prep.h's layouts)
// Nothing is allocated by an atomic counter: topology, boxes, leaf order and numbering are a function of the scene alone.
//
// Inter-workgroup visibility in stage 5 (eight XCDs with private L2s, per-CU L1s never refreshed by other CUs): a child's box is handed to the
// thread that arrives second at the parent, which may run on any CU.  Every word of a handed-over box is written with an agent-scope atomic
// store and read with an agent-scope atomic load (neither is served from a CU's L1 or left in one XCD's L2), and the arrival counter is an
// agent-scope acq_rel fetch-add: the first arrival's stores are released before its add, the second arrival's loads come after its own add has
// returned 1.  No plain load ever touches a word another workgroup wrote in the same launch.

namespace {
namespace dbuild {

using amber_bvh::Box;

constexpr uint32_t kNoParent = 0xffffffffu;

// Bounds are reduced with integer atomics on an order-preserving image of the binary32 value (min / max commute: no arrival order in the result).
__device__ __forceinline__ uint32_t FloatKey(float f) { const uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__host__ __device__ __forceinline__ float KeyFloat(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float f; memcpy(&f, &u, 4); return f;
}

struct Reduced {                 // keys (FloatKey) of running minima / maxima; then what the host reads back
  uint32_t raw_mn[3], raw_mx[3];   // geometric object boxes
  uint32_t wid_mn[3], wid_mx[3];   // widened object boxes (FlatBvh::bounds_min / bounds_max)
  uint32_t cen_mn[3], cen_mx[3];   // their centres
  uint32_t depth;                  // inner nodes on the longest way from the root to a leaf (db_boxes)
  uint32_t n_live;                 // inner nodes that survive the leaf collapse (db_count)
  uint32_t rmin;                   // key of the smallest |radius| over the spheres (3.0e38 without one): SetBvhRayMargin
  uint32_t bad_index;              // amber_hip_pt_update_objects: the first object whose new record may not replace the resident one (kNoParent: none)
};

__global__ void db_init(Reduced* r) {
  if (threadIdx.x < 3) {
    const uint32_t hi = FloatKey(3.0e38f), lo = FloatKey(-3.0e38f);     // Box::reset
    r->raw_mn[threadIdx.x] = hi; r->raw_mx[threadIdx.x] = lo; r->wid_mn[threadIdx.x] = hi; r->wid_mx[threadIdx.x] = lo;
    r->cen_mn[threadIdx.x] = hi; r->cen_mx[threadIdx.x] = lo;
  }
  if (threadIdx.x == 0) { r->depth = 0; r->n_live = 0; r->rmin = FloatKey(3.0e38f); r->bad_index = kNoParent; }
}

// min / max over the wave (every lane takes part: the callers keep out-of-range threads alive with neutral values), then one atomic per wave.
// A NaN bound is skipped, as Box::grow skips it (std::min / std::max keep their first argument).
__device__ __forceinline__ void ReduceBounds(const float mn[3], const float mx[3], bool valid, uint32_t* out_mn, uint32_t* out_mx) {
  for (int c = 0; c < 3; c++) {
    uint32_t kmn = valid && mn[c] == mn[c] ? FloatKey(mn[c]) : 0xffffffffu;
    uint32_t kmx = valid && mx[c] == mx[c] ? FloatKey(mx[c]) : 0u;
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t a = static_cast<uint32_t>(__shfl_xor(static_cast<int>(kmn), o)), b = static_cast<uint32_t>(__shfl_xor(static_cast<int>(kmx), o));
      kmn = a < kmn ? a : kmn; kmx = b > kmx ? b : kmx;
    }
    if ((threadIdx.x & 63u) == 0u) {
      if (kmn != 0xffffffffu) atomicMin(out_mn + c, kmn);
      if (kmx != 0u) atomicMax(out_mx + c, kmx);
    }
  }
}

__global__ void __launch_bounds__(256) db_bounds_raw(const DevObject* __restrict__ objs, uint32_t n, Reduced* r) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  Box b; b.reset();
  float radius = 3.0e38f;                                      // std::min(rmin, |radius|) as the host folds it: a NaN or an infinity never becomes the minimum
  if (i < n) {
    b = amber_bvh::ObjectBox(objs[i]);
    if ((objs[i].kind & 0xffu) == 1u && fabsf(objs[i].radius) < 3.0e38f) radius = fabsf(objs[i].radius);
  }
  ReduceBounds(b.mn, b.mx, i < n, r->raw_mn, r->raw_mx);
  uint32_t key = FloatKey(radius);
  for (int o = 32; o > 0; o >>= 1) { const uint32_t a = static_cast<uint32_t>(__shfl_xor(static_cast<int>(key), o)); key = a < key ? a : key; }
  if ((threadIdx.x & 63u) == 0u && key != FloatKey(3.0e38f)) atomicMin(&r->rmin, key);
}

// The scene figures BuildBvh derives from the geometric bounds: 16 eps D^2 (sphere slack) and D (triangle reach)
__device__ __forceinline__ void SceneSlack(const Reduced* r, double slack_factor, double& sphere_slack2, double& scene_diag) {
  double d2 = 0;
  for (int c = 0; c < 3; c++) { const double e = double(KeyFloat(r->raw_mx[c])) - KeyFloat(r->raw_mn[c]); d2 += e * e; }
  sphere_slack2 = slack_factor * 5.9604644775390625e-08 * d2;
  scene_diag = sqrt(d2);
}

__global__ void __launch_bounds__(256) db_bounds_wide(const DevObject* __restrict__ objs, uint32_t n, Reduced* r, double slack_factor, Box* __restrict__ boxes) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  double slack2, diag;
  SceneSlack(r, slack_factor, slack2, diag);                 // (raw_* are final: written by the previous launch)
  Box b; b.reset();
  float cen[3] = {0.f, 0.f, 0.f};
  if (i < n) {
    b = amber_bvh::ObjectBox(objs[i], slack2, diag);
    boxes[i] = b;
    for (int c = 0; c < 3; c++) cen[c] = 0.5f * (b.mn[c] + b.mx[c]);
  }
  ReduceBounds(b.mn, b.mx, i < n, r->wid_mn, r->wid_mx);
  ReduceBounds(cen, cen, i < n, r->cen_mn, r->cen_mx);
}

// 21 bits of x, y, z interleaved (x highest): 63-bit Morton code
__device__ __forceinline__ unsigned long long Spread21(unsigned long long v) {
  v &= 0x1fffffull;
  v = (v | v << 32) & 0x1f00000000ffffull;
  v = (v | v << 16) & 0x1f0000ff0000ffull;
  v = (v | v << 8) & 0x100f00f00f00f00full;
  v = (v | v << 4) & 0x10c30c30c30c30c3ull;
  v = (v | v << 2) & 0x1249249249249249ull;
  return v;
}
__global__ void __launch_bounds__(256) db_morton(const Box* __restrict__ boxes, uint32_t n, const Reduced* r, unsigned long long* __restrict__ codes, uint32_t* __restrict__ index) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  unsigned long long code = 0;
  for (int c = 0; c < 3; c++) {
    const double lo = KeyFloat(r->cen_mn[c]), hi = KeyFloat(r->cen_mx[c]);
    const double x = (double(0.5f * (boxes[i].mn[c] + boxes[i].mx[c])) - lo) / (hi - lo);     // NaN on an axis without extent (or a NaN centre): cell 0
    const unsigned long long cell = x > 0.0 ? (x < 1.0 ? static_cast<unsigned long long>(x * 2097152.0) : 2097151ull) : 0ull;
    code |= Spread21(cell < 2097151ull ? cell : 2097151ull) << (2 - c);
  }
  codes[i] = code; index[i] = i;
}

// Length of the common prefix of the keys at sorted positions i and j; -1 outside the array.  The key is the code's TOP 3 * kHierarchyBits bits
// followed by the position (unique).  The objects are sorted by all 63 bits, but the hierarchy follows the code only down to cells of 2^-8 of
// the centre bounds and halves the sorted order below that: on a surface (a terrain: a 2-D sheet in 3-D cells) a path of the full radix tree
// takes up to three levels per halving of the cell -- the 1M-triangle terrain came out deeper than the traversal's limit -- while a cell of
// k objects split by position is log2 k + 1 deep.  So depth <= 24 + log2(objects of the fullest cell) + 1, and the leaves of a cell are
// still runs of the Morton order.
constexpr int kHierarchyBits = 8;
__device__ __forceinline__ int Delta(const unsigned long long* __restrict__ codes, int n, int i, int j) {
  if (j < 0 || j >= n) return -1;
  const unsigned long long a = codes[i] >> (63 - 3 * kHierarchyBits), b = codes[j] >> (63 - 3 * kHierarchyBits);
  return a != b ? __clzll(static_cast<long long>(a ^ b)) : 64 + __clz(i ^ j);
}

// Karras, "Maximizing parallelism in the construction of BVHs, octrees and k-d trees" (2012), section 4: inner node i covers the sorted
// positions [first, last] and splits them behind position `split`.  A child reference is an inner node index, or ~position of a single object.
__global__ void __launch_bounds__(256) db_hierarchy(const unsigned long long* __restrict__ codes, uint32_t n, int32_t* __restrict__ left, int32_t* __restrict__ right,
                                                    uint32_t* __restrict__ first_of, uint32_t* __restrict__ last_of, uint32_t* __restrict__ parent_of_node, uint32_t* __restrict__ parent_of_object) {
  const int i = static_cast<int>(blockIdx.x * 256u + threadIdx.x), N = static_cast<int>(n);
  if (i >= N - 1) return;
  const int d = Delta(codes, N, i, i + 1) > Delta(codes, N, i, i - 1) ? 1 : -1;
  const int dmin = Delta(codes, N, i, i - d);
  long long lmax = 2;
  while (i + lmax * d >= 0 && i + lmax * d < N && Delta(codes, N, i, static_cast<int>(i + lmax * d)) > dmin) lmax *= 2;
  long long l = 0;
  for (long long t = lmax / 2; t >= 1; t /= 2) {
    const long long j = i + (l + t) * d;
    if (j >= 0 && j < N && Delta(codes, N, i, static_cast<int>(j)) > dmin) l += t;
  }
  const int j = static_cast<int>(i + l * d);
  const int dnode = Delta(codes, N, i, j);
  long long s = 0;
  for (long long t = (l + 1) / 2;; t = (t + 1) / 2) {
    const long long k = i + (s + t) * d;
    if (k >= 0 && k < N && Delta(codes, N, i, static_cast<int>(k)) > dnode) s += t;
    if (t <= 1) break;
  }
  const int split = static_cast<int>(i + s * d) + (d < 0 ? -1 : 0);
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  const int32_t l_ref = lo == split ? ~split : split, r_ref = hi == split + 1 ? ~(split + 1) : split + 1;
  left[i] = l_ref; right[i] = r_ref; first_of[i] = static_cast<uint32_t>(lo); last_of[i] = static_cast<uint32_t>(hi);
  if (l_ref >= 0) parent_of_node[l_ref] = static_cast<uint32_t>(i); else parent_of_object[~l_ref] = static_cast<uint32_t>(i);
  if (r_ref >= 0) parent_of_node[r_ref] = static_cast<uint32_t>(i); else parent_of_object[~r_ref] = static_cast<uint32_t>(i);
  if (i == 0) parent_of_node[0] = kNoParent;
}

// The box of one child as its parent keeps it until db_emit: 8 words {mn[3], mx[3], height, 0}.  height: inner nodes that survive the leaf
// collapse on the longest way from this child down to a leaf, the child included (0 for a subtree of at most kLeafSize objects).
typedef uint32_t __attribute__((address_space(1))) GlobalWord;
__device__ __forceinline__ void PublishWord(uint32_t* p, uint32_t v) { __hip_atomic_store((GlobalWord*)(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t ConsumeWord(uint32_t* p) { return __hip_atomic_load((GlobalWord*)(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(256) db_boxes(const Box* __restrict__ boxes, const uint32_t* __restrict__ sorted_index, uint32_t n, const int32_t* __restrict__ left,
                                                const uint32_t* __restrict__ first_of, const uint32_t* __restrict__ last_of, const uint32_t* __restrict__ parent_of_node,
                                                const uint32_t* __restrict__ parent_of_object, uint32_t* child_boxes /* [n - 1][2][8] */, uint32_t* arrivals /* [n - 1], zero */, Reduced* r) {
  const uint32_t pos = blockIdx.x * 256u + threadIdx.x;
  if (pos >= n) return;
  // The carried box is built as the host builder builds every box -- reset, then grow with the accumulator first -- so a NaN bound of an object
  // (a NaN centre or radius: create accepts such scenes, no ray hits the object) is skipped, never carried: std::min / std::max keep their FIRST
  // argument on NaN, so a NaN already IN the accumulator would swallow every finite bound merged later, and which thread carries it depends on the
  // arrival order.  A published box therefore never holds a NaN, and the unions are a function of the scene alone.
  Box b; b.reset(); b.grow(boxes[sorted_index[pos]]);
  uint32_t height = 0;
  uint32_t node = parent_of_object[pos];
  uint32_t side = left[node] == ~static_cast<int32_t>(pos) ? 0u : 1u;
  for (uint32_t level = 0; level < 128u; level++) {          // (a radix tree over 96-bit keys has at most 96 levels)
    uint32_t* mine = child_boxes + (static_cast<size_t>(node) * 2u + side) * 8u;
    for (int c = 0; c < 3; c++) { PublishWord(mine + c, __float_as_uint(b.mn[c])); PublishWord(mine + 3 + c, __float_as_uint(b.mx[c])); }
    PublishWord(mine + 6, height);
    const uint32_t before = __hip_atomic_fetch_add((GlobalWord*)(arrivals + node), 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (before == 0u) return;                                // the sibling subtree is not finished: its last thread will continue from here
    uint32_t* theirs = child_boxes + (static_cast<size_t>(node) * 2u + (side ^ 1u)) * 8u;
    Box o;
    for (int c = 0; c < 3; c++) { o.mn[c] = __uint_as_float(ConsumeWord(theirs + c)); o.mx[c] = __uint_as_float(ConsumeWord(theirs + 3 + c)); }
    const uint32_t their_height = ConsumeWord(theirs + 6);
    b.grow(o);
    const bool live = last_of[node] - first_of[node] + 1u > static_cast<uint32_t>(amber_bvh::kLeafSize);
    height = live ? (height > their_height ? height : their_height) + 1u : 0u;
    const uint32_t parent = parent_of_node[node];
    if (parent == kNoParent) { r->depth = height; return; }   // the root: read by the host after the launch
    side = left[parent] == static_cast<int32_t>(node) ? 0u : 1u;
    node = parent;
  }
}

// 1 for the inner nodes that stay inner nodes; their inclusive scan numbers them (node 0, the root, first)
__global__ void __launch_bounds__(256) db_live(const uint32_t* __restrict__ first_of, const uint32_t* __restrict__ last_of, uint32_t n_inner, uint32_t* __restrict__ live) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n_inner) live[i] = last_of[i] - first_of[i] + 1u > static_cast<uint32_t>(amber_bvh::kLeafSize) ? 1u : 0u;
}
__global__ void db_count(const uint32_t* __restrict__ rank, uint32_t n_inner, Reduced* r) { r->n_live = rank[n_inner - 1u]; }

struct Grid { float gmin[3], step[3], extent; };

// Leaf reference of the sorted positions [first, first + count): first * 16 + all_triangles * 8 + all_spheres * 4 + count (QuantizedLeafRef)
__device__ __forceinline__ int32_t LeafRef(const DevObject* __restrict__ objs, const uint32_t* __restrict__ sorted_index, uint32_t first, uint32_t count) {
  bool spheres = count > 0u, tris = count > 0u;
  for (uint32_t k = 0; k < count; k++) { const uint32_t kind = objs[sorted_index[first + k]].kind & 0xffu; spheres = spheres && kind == 1u; tris = tris && kind == 0u; }
#if !AMBER_BVH_TRI_LEAVES
  tris = false;
#endif
  return -static_cast<int32_t>(first * 16u + (tris ? 8u : 0u) + (spheres ? 4u : 0u) + count) - 1;
}

__global__ void __launch_bounds__(256) db_emit(const DevObject* __restrict__ objs, const uint32_t* __restrict__ sorted_index, uint32_t n_inner, const int32_t* __restrict__ left,
                                               const int32_t* __restrict__ right, const uint32_t* __restrict__ first_of, const uint32_t* __restrict__ last_of,
                                               const uint32_t* __restrict__ rank, const uint32_t* __restrict__ child_boxes, Grid g, DevBvhNodeQ* __restrict__ nodes, uint32_t n_nodes) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_inner) return;
  const uint32_t kLeaf = static_cast<uint32_t>(amber_bvh::kLeafSize);
  if (last_of[i] - first_of[i] + 1u <= kLeaf) return;        // inside a leaf
  const uint32_t me = rank[i] - 1u;
  if (me >= n_nodes) return;                                 // (cannot happen: n_nodes is the scan's total)
  DevBvhNodeQ q;
  for (uint32_t side = 0; side < 2u; side++) {
    const uint32_t* w = child_boxes + (static_cast<size_t>(i) * 2u + side) * 8u;      // plain loads: written by an earlier launch
    Box b;
    for (int c = 0; c < 3; c++) { b.mn[c] = __uint_as_float(w[c]); b.mx[c] = __uint_as_float(w[3 + c]); }
    amber_bvh::PadBox(b, g.extent);
    for (int c = 0; c < 3; c++) q.w[3 * side + c] = amber_bvh::PlaneWordOutward(b.mn[c], b.mx[c], g.gmin[c], g.step[c]);
    const int32_t ref = side ? right[i] : left[i];
    int32_t out;
    if (ref < 0) out = LeafRef(objs, sorted_index, static_cast<uint32_t>(~ref), 1u);
    else {
      const uint32_t count = last_of[ref] - first_of[ref] + 1u;
      out = count <= kLeaf ? LeafRef(objs, sorted_index, first_of[ref], count) : static_cast<int32_t>(rank[ref] - 1u);
    }
    if (side) q.right = out; else q.left = out;
  }
  nodes[me] = q;
}

__global__ void __launch_bounds__(256) db_gather(const DevObject* __restrict__ objs, const uint32_t* __restrict__ sorted_index, uint32_t n, uint32_t* __restrict__ prims,
                                                 DevObject* __restrict__ leaf_objects, float4* __restrict__ leaf_spheres, float4* __restrict__ leaf_tris /* null: no triangles */) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const uint32_t scene_index = sorted_index[k];
  const DevObject ob = objs[scene_index];
  if (prims) prims[k] = scene_index;                         // (null: a refit gathers through the leaf order it keeps)
  leaf_objects[k] = ob;
  const uint32_t kind = ob.kind & 0xffu;
  leaf_spheres[k] = kind == 1u ? make_float4(ob.a[0], ob.a[1], ob.a[2], ob.radius) : make_float4(0.f, 0.f, 0.f, 0.f);
  if (leaf_tris) {
    const bool tri = kind == 0u;
    leaf_tris[3 * k] = tri ? make_float4(ob.a[0], ob.a[1], ob.a[2], ob.e1[0]) : make_float4(0.f, 0.f, 0.f, 0.f);
    leaf_tris[3 * k + 1] = tri ? make_float4(ob.e1[1], ob.e1[2], ob.e2[0], ob.e2[1]) : make_float4(0.f, 0.f, 0.f, 0.f);
    leaf_tris[3 * k + 2] = tri ? make_float4(ob.e2[2], __uint_as_float(scene_index), 0.f, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// What the build needs to know of the scene besides the device records: figures of the object KINDS (which an update never changes) and the
// smallest sphere radius when the caller has it (create: from the host records; an update: db_bounds_raw reduces it).
struct BuildInput {
  const DevObject* objs; uint32_t n;
  bool any_tri, has_spheres, rmin_known; float rmin;
  uint32_t small_kinds[3];         // kinds of the first three objects (a scene that is one leaf)
  bool prepared;                   // the caller has run db_init on the scratch's Reduced and enqueued what writes objs (and may set bad_index)
};
constexpr uint32_t kReasonRejected = 0xffu;   // internal to an update: Reduced.bad_index names a record that was refused
struct BuildResult { uint32_t reason, n_nodes, depth; Reduced red; };

// The grid of the plane words, as QuantizedBvh's fields.  Every child box lies inside the bounds of all widened boxes and PadBox is monotone (a
// box inside another is padded by no more, from no smaller a minimum), so the padded bounds contain every padded child box: the grid QuantizeBvh
// derives from the node boxes themselves is at most that large.
inline Grid GridOfBounds(const float bmn[3], const float bmx[3], bool tree, DevScene& sc) {
  Grid g{};
  Box all; for (int c = 0; c < 3; c++) { all.mn[c] = bmn[c]; all.mx[c] = bmx[c]; }
  g.extent = std::max(all.mx[0] - all.mn[0], std::max(all.mx[1] - all.mn[1], all.mx[2] - all.mn[2]));
  if (tree) {
    Box padded = all;
    amber_bvh::PadBox(padded, g.extent);
    for (int c = 0; c < 3; c++) {
      float mid, half;
      amber_bvh::F16AxisGrid(padded.mn[c], padded.mx[c], mid, half);
      g.gmin[c] = mid; g.step[c] = half;
      sc.bvh_gmin[c] = mid; sc.bvh_step[c] = half; sc.bvh_reach[c] = static_cast<float>(double(half) * 1.002);    // |value| <= 1 + one binary16 step
    }
  } else {
    for (int c = 0; c < 3; c++) { sc.bvh_gmin[c] = 0.f; sc.bvh_step[c] = 1.f; sc.bvh_reach[c] = 0.f; }           // QuantizedBvh's defaults: no node reads them
  }
  return g;
}
inline bool FiniteBounds(const Reduced& red, float bmn[3], float bmx[3]) {
  for (int c = 0; c < 3; c++) { bmn[c] = KeyFloat(red.wid_mn[c]); bmx[c] = KeyFloat(red.wid_mx[c]); }
  for (int c = 0; c < 3; c++)
    if (!(std::fabs(bmn[c]) < 3.0e38f && std::fabs(bmx[c]) < 3.0e38f && bmn[c] <= bmx[c])) return false;
  return true;
}

}  // namespace dbuild

// Builds the tree of the in.n objects at in.objs (device memory) into the handle's arrays (h->tree; the node array is replaced when the tree has
// more nodes than it holds, the others are allocated once) and sets the DevScene fields that describe it.  res->reason != 0 on return: nothing
// of the handle was changed (create then builds on the host, an update refits or refuses).
int DeviceBuildBvh(amber_hip_pt* h, const dbuild::BuildInput& in, BvhBuildScratch& s, dbuild::BuildResult* res) {
  using namespace dbuild;
  res->reason = AMBER_BUILD_REASON_NONE;
  const uint32_t n = in.n, n_inner = n - 1u;
  const uint32_t kLeaf = static_cast<uint32_t>(amber_bvh::kLeafSize);
  const bool tree = n > kLeaf;                               // else the whole scene is one leaf
  const hipStream_t st = h->stream;
  const dim3 by_object((n + 255u) / 256u), by_node((n_inner + 255u) / 256u), wg(256);
  double slack_factor = 16.0;
  if (const char* env = std::getenv("AMBER_BVH_SPHERE_SLACK")) slack_factor = std::atof(env);   // BuildBvh's test hook

  HIP_TRY(s.red.need(1)); HIP_TRY(s.boxes.need(n)); HIP_TRY(s.codes.need(n)); HIP_TRY(s.codes_sorted.need(n)); HIP_TRY(s.index.need(n)); HIP_TRY(s.sorted.need(n));
  size_t temp_bytes = 0;
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, temp_bytes, s.codes.p, s.codes_sorted.p, s.index.p, s.sorted.p, n, 0u, 63u, st));
  size_t scan_bytes = 0;
  if (tree) {
    HIP_TRY(s.left.need(n_inner)); HIP_TRY(s.right.need(n_inner)); HIP_TRY(s.first.need(n_inner)); HIP_TRY(s.last.need(n_inner));
    HIP_TRY(s.parent_node.need(n_inner)); HIP_TRY(s.parent_object.need(n)); HIP_TRY(s.child_boxes.need(static_cast<size_t>(n_inner) * 16u));
    HIP_TRY(s.arrivals.need(n_inner)); HIP_TRY(s.live.need(n_inner)); HIP_TRY(s.rank.need(n_inner));
    HIP_TRY(rocprim::inclusive_scan(nullptr, scan_bytes, s.live.p, s.rank.p, n_inner, rocprim::plus<uint32_t>(), st));
  }
  HIP_TRY(s.temp.need(std::max(temp_bytes, scan_bytes)));

  if (!in.prepared) hipLaunchKernelGGL(db_init, dim3(1), dim3(64), 0, st, s.red.p);
  hipLaunchKernelGGL(db_bounds_raw, by_object, wg, 0, st, in.objs, n, s.red.p);
  hipLaunchKernelGGL(db_bounds_wide, by_object, wg, 0, st, in.objs, n, s.red.p, slack_factor, s.boxes.p);
  hipLaunchKernelGGL(db_morton, by_object, wg, 0, st, s.boxes.p, n, s.red.p, s.codes.p, s.index.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(rocprim::radix_sort_pairs(s.temp.p, temp_bytes, s.codes.p, s.codes_sorted.p, s.index.p, s.sorted.p, n, 0u, 63u, st));
  if (tree) {
    HIP_TRY(hipMemsetAsync(s.arrivals.p, 0, static_cast<size_t>(n_inner) * sizeof(uint32_t), st));
    hipLaunchKernelGGL(db_hierarchy, by_node, wg, 0, st, s.codes_sorted.p, n, s.left.p, s.right.p, s.first.p, s.last.p, s.parent_node.p, s.parent_object.p);
    hipLaunchKernelGGL(db_boxes, by_object, wg, 0, st, s.boxes.p, s.sorted.p, n, s.left.p, s.first.p, s.last.p, s.parent_node.p, s.parent_object.p, s.child_boxes.p, s.arrivals.p, s.red.p);
    hipLaunchKernelGGL(db_live, by_node, wg, 0, st, s.first.p, s.last.p, n_inner, s.live.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(rocprim::inclusive_scan(s.temp.p, scan_bytes, s.live.p, s.rank.p, n_inner, rocprim::plus<uint32_t>(), st));
    hipLaunchKernelGGL(db_count, dim3(1), dim3(1), 0, st, s.rank.p, n_inner, s.red.p);
    HIP_TRY(hipGetLastError());
  }
  Reduced& red = res->red;
  HIP_TRY(hipMemcpyAsync(&red, s.red.p, sizeof red, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));

  if (red.bad_index != kNoParent) { res->reason = kReasonRejected; return AMBER_OK; }
  float bmn[3], bmx[3];
  if (!FiniteBounds(red, bmn, bmx)) { res->reason = AMBER_BUILD_REASON_BOUNDS; return AMBER_OK; }
  const uint32_t depth = tree ? red.depth : 0u, n_nodes = tree ? red.n_live : 0u;
  const uint32_t max_depth = h->env.test_device_build_max_depth ? std::min(h->env.test_device_build_max_depth, static_cast<uint32_t>(amber_bvh::kMaxDepth))
                                                                : static_cast<uint32_t>(amber_bvh::kMaxDepth);
  if (depth > max_depth) { res->reason = AMBER_BUILD_REASON_DEPTH; return AMBER_OK; }   // never traversed: the stacks assume the limit
  if (tree && (n_nodes == 0u || n_nodes > n_inner)) return Fail(AMBER_EHIP, "device BVH build: inconsistent node count " + std::to_string(n_nodes));

  // the arrays first (the + 1 / + 3: no array is empty on the device, as in create's uploads): a failure here leaves the handle as it was.  The
  // arrays may be in use by passes enqueued earlier; everything below is ordered behind them on the handle's stream, and the stream has just been waited for.
  // A node array that is too small is not replaced before everything that can fail has been enqueued: until then the handle's tree stands.
  BvhTreeBufs& t = h->tree;
  DevBuf<uint8_t> larger_nodes;
  const bool grow_nodes = !t.nodes.p || t.nodes.n < (n_nodes + 1u) * sizeof(DevBvhNodeQ);
  if (grow_nodes) HIP_TRY(larger_nodes.alloc((n_nodes + 1u) * sizeof(DevBvhNodeQ)));
  HIP_TRY(t.prims.need((n + 1u) * sizeof(uint32_t)));
  HIP_TRY(t.tris.need(((in.any_tri ? 3u * static_cast<size_t>(n) : 0u) + 3u) * sizeof(float4)));
  HIP_TRY(t.objects.need((n + 1u) * sizeof(DevObject)));
  HIP_TRY(t.spheres.need((n + 1u) * sizeof(float4)));
  DevBvhNodeQ* d_nodes = reinterpret_cast<DevBvhNodeQ*>(grow_nodes ? larger_nodes.p : t.nodes.p); uint32_t* d_prims = reinterpret_cast<uint32_t*>(t.prims.p);
  DevObject* d_leaf_objects = reinterpret_cast<DevObject*>(t.objects.p); float4* d_spheres = reinterpret_cast<float4*>(t.spheres.p); float4* d_tris = reinterpret_cast<float4*>(t.tris.p);

  DevScene& sc = h->scene;
  const Grid g = GridOfBounds(bmn, bmx, tree, sc);
  amber_prep::SetBvhRayMargin(sc, bmn, bmx, in.has_spheres, in.has_spheres ? (in.rmin_known ? in.rmin : KeyFloat(red.rmin)) : 0.0f);

  if (tree) hipLaunchKernelGGL(db_emit, by_node, wg, 0, st, in.objs, s.sorted.p, n_inner, s.left.p, s.right.p, s.first.p, s.last.p, s.rank.p, s.child_boxes.p, g, d_nodes, n_nodes);
  hipLaunchKernelGGL(db_gather, by_object, wg, 0, st, in.objs, s.sorted.p, n, d_prims, d_leaf_objects, d_spheres, in.any_tri ? d_tris : nullptr);
  HIP_TRY(hipGetLastError());
  if (tree) sc.bvh_root = 0;
  else {                                                     // one leaf over the sorted order: read it back (at most kLeafSize words) for the leaf's kind bits
    uint32_t order[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(order, s.sorted.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    sc.bvh_root = amber_bvh::QuantizedLeafRef(amber_bvh::Builder::LeafRef(0u, n), [&](uint32_t slot) { return in.small_kinds[order[slot] < 3u ? order[slot] : 0u]; });
  }
  if (!in.prepared) HIP_TRY(hipStreamSynchronize(st));        // create's scratch goes out of scope when it returns; an update keeps its scratch and waits once, at its end
  if (grow_nodes) { t.nodes.swap(larger_nodes); s.retired_nodes.swap(larger_nodes); }   // (what retired_nodes held before is released here: an update has waited for the stream since)
  sc.bvh_nodes = d_nodes; sc.bvh_prims = d_prims; sc.bvh_tris = d_tris; sc.bvh_objects = d_leaf_objects; sc.bvh_spheres = d_spheres;
  res->n_nodes = n_nodes; res->depth = depth;
  return AMBER_OK;
}

}  // namespace

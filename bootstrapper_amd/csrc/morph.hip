// `bs refine morph` on the device (reference refine.py:310-360 `_apply_morph` / `_morph_block`, which calls fastmorph; that
// package is absent here, so the rule is the one written out in DESIGN.md section 7g and include/bsmi.h, parity unpinned).
//
// Stencil ops (dilate, erode) on a u64 label volume: a workgroup of 256 stages a tile of 8 x 8 x 32 voxels and its halo of one
// voxel in LDS (positions outside the array read as 0) and every lane walks the 8 voxels of its column along z with the stencil
// in registers: two of the three 3 x 3 planes carry over from one voxel to the next, so a voxel costs 9 LDS reads, not 27.
// A voxel that keeps its value (non-zero under dilate, zero under erode) and a stencil that holds one id need no counting;
// a background voxel with labelled neighbours takes the most frequent of them by compare-and-count over the 26 (8) values,
// fully unrolled, every value and every count in a register (no private array is indexed at run time).
// Traffic: 8 B read + 8 B written per voxel and iteration from HBM (the halo re-reads are served by L2).
//
// fill_holes: connected components of equal id by union-find over the voxels (a label-equality variant: the component
// labelling behind bsmi_cc_affs_u8 wants u8 affinities and a bsmi_seg handle, whose work space is sized for blocks of the
// watershed, not for a 2048^2 read block), a flag per component for "touches a face", a table of face counts per (component,
// neighbouring id) for the others, the decision on the host from the read-out table, and one pass that writes the result.
#include <hip/hip_runtime.h>

#include <unordered_map>

#include "../../include/bsmi.h"
#include "common.h"
#include "u64_table.h"

namespace bsmi {
namespace {

constexpr int kTX = 32, kTY = 8, kTZ = 8;

// the most frequent non-zero value of v[0..N), ties to the smallest; 0 if there is none
template <int N>
__device__ __forceinline__ uint64_t mode_nonzero(const uint64_t (&v)[N]) {
  int cnt[N];
#pragma unroll
  for (int i = 0; i < N; ++i) cnt[i] = 1;
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int j = i + 1; j < N; ++j) {
      const int e = v[i] == v[j] ? 1 : 0;
      cnt[i] += e;
      cnt[j] += e;
    }
  }
  uint64_t best = 0;
  int bc = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const bool take = v[i] != 0 && (cnt[i] > bc || (cnt[i] == bc && v[i] < best));
    best = take ? v[i] : best;
    bc = take ? cnt[i] : bc;
  }
  return best;
}

// one output voxel from its stencil s[0..N) (centre at N / 2; outside the array = 0)
template <int N, int OP>
__device__ __forceinline__ uint64_t morph_voxel(const uint64_t (&s)[N]) {
  const uint64_t c = s[N / 2];
  uint64_t any = 0;
  bool same = true;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    any |= s[i];
    same = same && s[i] == c;
  }
  if (OP == BSMI_MORPH_ERODE) return same ? c : 0;
  if (c != 0 || any == 0) return c;
  uint64_t o[N - 1];
#pragma unroll
  for (int i = 0; i < N - 1; ++i) o[i] = s[i < N / 2 ? i : i + 1];
  return mode_nonzero<N - 1>(o);
}

// grid: tiles in x-fastest order; block (kTX, kTY).  XY: every z section on its own (3 x 3 stencil, no halo along z)
template <bool XY, int OP>
__global__ void __launch_bounds__(kTX* kTY) label_morph_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, int D, int H, int W,
                                                               int tiles_x, int tiles_y) {
  constexpr int LZ = XY ? kTZ : kTZ + 2, LY = kTY + 2, LX = kTX + 2;
  __shared__ uint64_t tile[LZ * LY * LX];
  const int64_t b = blockIdx.x;
  const int bx = (int)(b % tiles_x), by = (int)(b / tiles_x % tiles_y), bz = (int)(b / ((int64_t)tiles_x * tiles_y));
  const int x0 = bx * kTX, y0 = by * kTY, z0 = bz * kTZ;
  const int tid = threadIdx.y * kTX + threadIdx.x;
  for (int i = tid; i < LZ * LY * LX; i += kTX * kTY) {
    const int lz = i / (LY * LX), r = i - lz * (LY * LX), ly = r / LX, lx = r - ly * LX;
    const int z = z0 + lz - (XY ? 0 : 1), y = y0 + ly - 1, x = x0 + lx - 1;
    const bool inside = z >= 0 && z < D && y >= 0 && y < H && x >= 0 && x < W;
    tile[i] = inside ? in[((int64_t)z * H + y) * W + x] : 0;
  }
  __syncthreads();
  const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
  if (x >= W || y >= H) return;
  const uint64_t* t = tile + threadIdx.y * LX + threadIdx.x;  // stencil corner (ly - 1, lx - 1) of plane 0
  if (XY) {
#pragma unroll
    for (int k = 0; k < kTZ; ++k) {
      if (z0 + k >= D) break;
      uint64_t s[9];
#pragma unroll
      for (int j = 0; j < 9; ++j) s[j] = t[(k * LY + j / 3) * LX + j % 3];
      out[((int64_t)(z0 + k) * H + y) * W + x] = morph_voxel<9, OP>(s);
    }
  } else {
    uint64_t s[27];
#pragma unroll
    for (int j = 0; j < 18; ++j) s[9 + j] = t[(j / 9 * LY + j % 9 / 3) * LX + j % 3];
#pragma unroll
    for (int k = 0; k < kTZ; ++k) {
      if (z0 + k >= D) break;
#pragma unroll
      for (int j = 0; j < 18; ++j) s[j] = s[9 + j];
#pragma unroll
      for (int j = 0; j < 9; ++j) s[18 + j] = t[((k + 2) * LY + j / 3) * LX + j % 3];
      out[((int64_t)(z0 + k) * H + y) * W + x] = morph_voxel<27, OP>(s);
    }
  }
}

// ---- fill_holes ----

// overflow bits of the flags word
constexpr uint32_t kOvfPairs = 1, kOvfIds = 2;

struct FillArgs {
  const uint64_t* in;
  uint64_t* out;
  uint32_t* parent;  // [n] union-find forest over the voxels; after cc_flatten_kernel: the smallest voxel index of the component
  uint8_t* touch;    // [n] touch[root] = 1: the component has a voxel on a face of the array (of its section with xy)
  uint64_t* id_keys;     // [cap + 1] neighbouring ids -> dense index (their slot)
  uint64_t* pair_keys;   // [cap] root << 32 | id slot
  unsigned long long* pair_counts;  // [cap] faces
  uint32_t* flags;   // [0] overflow bits, [1] pair inserts, [2] id inserts
  uint64_t cap;
  int D, H, W, xy;
  uint32_t n;
};

__device__ __forceinline__ uint32_t uf_find(uint32_t* p, uint32_t i) {
  for (;;) {
    const uint32_t q = __atomic_load_n(&p[i], __ATOMIC_RELAXED);
    if (q == i) return i;
    i = q;
  }
}

// roots only ever point to smaller indices, so the forest has no cycle and a component's root is its smallest voxel
// (seg_internal.h's cc_find / cc_unite are another algorithm -- int32_t parents, atomicMin -- and stay separate)
__device__ __forceinline__ void uf_unite(uint32_t* p, uint32_t a, uint32_t b) {
  for (;;) {
    a = uf_find(p, a);
    b = uf_find(p, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    if (atomicCAS(&p[a], a, b) == a) return;
  }
}

// a wave per 64-voxel segment of a row: every voxel starts under the first voxel of its run of equal ids in the segment
__global__ void __launch_bounds__(256) cc_init_kernel(FillArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t nseg = (a.W + 63) / 64;
  const int64_t items = (int64_t)a.D * a.H * nseg;
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x / 64);
  for (int64_t it = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); it < items; it += nwaves) {
    const int64_t row = it / nseg;
    const int x = (int)(it - row * nseg) * 64 + lane;
    const bool in = x < a.W;
    const uint64_t id = in ? a.in[row * a.W + x] : 0;
    const uint64_t prev = __shfl_up(id, 1);
    const bool head = lane == 0 || prev != id;
    const uint64_t heads = __ballot(head);
    const uint64_t upto = heads & (~0ull >> (63 - lane));  // heads at or before this lane (lane 0 is always one)
    const int first = 63 - __clzll((long long)upto);
    if (in) a.parent[row * a.W + x] = (uint32_t)(row * a.W + x - (lane - first));
  }
}

__global__ void __launch_bounds__(256) cc_union_kernel(FillArgs a) {
  const uint32_t plane = (uint32_t)a.H * (uint32_t)a.W;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t v = (uint32_t)i;
    const uint32_t x = v % (uint32_t)a.W, y = v / (uint32_t)a.W % (uint32_t)a.H;
    const uint64_t id = a.in[v];
    // along x the runs inside a 64-voxel segment are joined already: only a segment's first voxel looks left
    if (x > 0 && (x & 63) == 0 && a.in[v - 1] == id) uf_unite(a.parent, v, v - 1);
    if (y > 0 && a.in[v - a.W] == id) uf_unite(a.parent, v, v - (uint32_t)a.W);
    if (!a.xy && v >= plane && a.in[v - plane] == id) uf_unite(a.parent, v, v - plane);
  }
}

__global__ void __launch_bounds__(256) cc_flatten_kernel(FillArgs a) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t v = (uint32_t)i;
    const uint32_t r = uf_find(a.parent, v);
    __atomic_store_n(&a.parent[v], r, __ATOMIC_RELAXED);  // an ancestor for an ancestor: readers still reach the root
    const int x = (int)(v % (uint32_t)a.W), y = (int)(v / (uint32_t)a.W % (uint32_t)a.H), z = (int)(v / ((uint32_t)a.H * (uint32_t)a.W));
    const bool face = x == 0 || x == a.W - 1 || y == 0 || y == a.H - 1 || (!a.xy && (z == 0 || z == a.D - 1));
    if (face) a.touch[r] = 1;
  }
}

// faces between a voxel of an enclosed component and its neighbours of another id, counted per (component, neighbouring id)
__global__ void __launch_bounds__(256) fill_count_kernel(FillArgs a) {
  const int64_t plane = (int64_t)a.H * a.W;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t v = (uint32_t)i;
    const uint32_t r = a.parent[v];
    if (a.touch[r]) continue;
    // an enclosed component has no voxel on a face, so every neighbour lies inside the array
    const uint64_t id = a.in[v];
    auto face = [&](int64_t at) {
      const uint64_t nb = a.in[at];
      if (nb == id) return;
      const int64_t slot = nb == kEmpty ? (int64_t)a.cap : table_slot(a.id_keys, a.cap, nb, a.flags + 2, a.flags, kOvfIds);
      if (slot < 0) return;
      const int64_t p = table_slot(a.pair_keys, a.cap, (uint64_t)r << 32 | (uint64_t)slot, a.flags + 1, a.flags, kOvfPairs);
      if (p >= 0) atomicAdd(&a.pair_counts[p], 1ull);
    };
    face((int64_t)v - 1);
    face((int64_t)v + 1);
    face((int64_t)v - a.W);
    face((int64_t)v + a.W);
    if (!a.xy) {
      face((int64_t)v - plane);
      face((int64_t)v + plane);
    }
  }
}

// out = in, but the voxels of a component listed in (roots ascending, ids) take the listed id
__global__ void __launch_bounds__(256) fill_apply_kernel(FillArgs a, const uint64_t* roots, const uint64_t* ids, uint32_t m) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t v = (uint32_t)i;
    uint64_t id = a.in[v];
    const uint32_t r = a.parent[v];
    if (m && !a.touch[r]) {
      uint32_t lo = 0, hi = m;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (roots[mid] < r) lo = mid + 1; else hi = mid;
      }
      if (lo < m && roots[lo] == r) id = ids[lo];
    }
    a.out[v] = id;
  }
}

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace
}  // namespace bsmi

using namespace bsmi;

extern "C" {

int bsmi_label_morph_u64(int device, const uint64_t* in_dev, const int64_t shape[3], int op, int iterations, int xy, uint64_t* out_dev,
                         uint64_t* tmp_dev, void* stream) {
  if (!in_dev || !shape || !out_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (op != BSMI_MORPH_DILATE && op != BSMI_MORPH_ERODE) BSMI_FAIL(BSMI_ERR_INVALID, "op %d: BSMI_MORPH_DILATE or BSMI_MORPH_ERODE", op);
  if (iterations < 1 || iterations > 255) BSMI_FAIL(BSMI_ERR_INVALID, "iterations %d: 1..255", iterations);
  if (in_dev == out_dev || tmp_dev == in_dev || tmp_dev == out_dev) BSMI_FAIL(BSMI_ERR_INVALID, "in, out and tmp must be different buffers");
  if (iterations > 1 && !tmp_dev) BSMI_FAIL(BSMI_ERR_INVALID, "%d iterations need the ping-pong buffer tmp_dev", iterations);
  for (int d = 0; d < 3; ++d)
    if (shape[d] < 0 || shape[d] > (1 << 20)) BSMI_FAIL(BSMI_ERR_INVALID, "shape out of range on axis %d", d);
  const int D = (int)shape[0], H = (int)shape[1], W = (int)shape[2];
  if (D == 0 || H == 0 || W == 0) return BSMI_OK;
  const int tx = ceil_div(W, kTX), ty = ceil_div(H, kTY), tz = ceil_div(D, kTZ);
  const int64_t tiles = (int64_t)tx * ty * tz;
  if (tiles >= (1ll << 31)) BSMI_FAIL(BSMI_ERR_INVALID, "volume too large for one call (%lld tiles)", (long long)tiles);
  BSMI_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)tiles), blk(kTX, kTY);
  const uint64_t* src = in_dev;
  for (int it = 0; it < iterations; ++it) {
    // the last iteration lands in out_dev, the ones before it alternate between the two buffers
    uint64_t* dst = (iterations - 1 - it) % 2 == 0 ? out_dev : tmp_dev;
    if (xy && op == BSMI_MORPH_DILATE)
      hipLaunchKernelGGL((label_morph_kernel<true, BSMI_MORPH_DILATE>), grid, blk, 0, s, src, dst, D, H, W, tx, ty);
    else if (xy)
      hipLaunchKernelGGL((label_morph_kernel<true, BSMI_MORPH_ERODE>), grid, blk, 0, s, src, dst, D, H, W, tx, ty);
    else if (op == BSMI_MORPH_DILATE)
      hipLaunchKernelGGL((label_morph_kernel<false, BSMI_MORPH_DILATE>), grid, blk, 0, s, src, dst, D, H, W, tx, ty);
    else
      hipLaunchKernelGGL((label_morph_kernel<false, BSMI_MORPH_ERODE>), grid, blk, 0, s, src, dst, D, H, W, tx, ty);
    src = dst;
  }
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

size_t bsmi_label_fill_holes_scratch_bytes(const int64_t shape[3], uint64_t table_capacity) {
  if (!shape) return 0;
  const size_t n = (size_t)shape[0] * shape[1] * shape[2];
  return align256(n * sizeof(uint32_t)) + align256(n) + align256((table_capacity + 1) * sizeof(uint64_t)) +
         2 * align256(table_capacity * sizeof(uint64_t)) + 256;
}

int bsmi_label_fill_holes_u64(int device, const uint64_t* in_dev, const int64_t shape[3], int xy, uint64_t* out_dev, void* scratch_dev,
                              size_t scratch_bytes, uint64_t table_capacity, uint64_t* n_filled, void* stream) {
  if (!in_dev || !shape || !out_dev || !scratch_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (in_dev == out_dev) BSMI_FAIL(BSMI_ERR_INVALID, "in and out must be different buffers");
  if (table_capacity < 2 || table_capacity > (1ull << 31) || (table_capacity & (table_capacity - 1)))
    BSMI_FAIL(BSMI_ERR_INVALID, "table_capacity %llu: a power of two in [2, 2^31]", (unsigned long long)table_capacity);
  for (int d = 0; d < 3; ++d)
    if (shape[d] < 0 || shape[d] > (1 << 20)) BSMI_FAIL(BSMI_ERR_INVALID, "shape out of range on axis %d", d);
  const uint64_t n64 = (uint64_t)shape[0] * shape[1] * shape[2];
  if (n64 >= 0xffffffffull) BSMI_FAIL(BSMI_ERR_INVALID, "%llu voxels: fill_holes takes fewer than 2^32 - 1 in one call", (unsigned long long)n64);
  if (scratch_bytes < bsmi_label_fill_holes_scratch_bytes(shape, table_capacity))
    BSMI_FAIL(BSMI_ERR_INVALID, "scratch of %zu bytes: bsmi_label_fill_holes_scratch_bytes asks for %zu", scratch_bytes,
              bsmi_label_fill_holes_scratch_bytes(shape, table_capacity));
  if (n_filled) *n_filled = 0;
  if (n64 == 0) return BSMI_OK;
  BSMI_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)n64, cap = (size_t)table_capacity;
  FillArgs a{};
  char* base = (char*)scratch_dev;
  a.parent = (uint32_t*)base;
  base += align256(n * sizeof(uint32_t));
  a.touch = (uint8_t*)base;
  base += align256(n);
  a.id_keys = (uint64_t*)base;
  base += align256((cap + 1) * sizeof(uint64_t));
  a.pair_keys = (uint64_t*)base;
  base += align256(cap * sizeof(uint64_t));
  a.pair_counts = (unsigned long long*)base;
  base += align256(cap * sizeof(uint64_t));
  a.flags = (uint32_t*)base;
  a.in = in_dev;
  a.out = out_dev;
  a.cap = cap;
  a.D = (int)shape[0];
  a.H = (int)shape[1];
  a.W = (int)shape[2];
  a.xy = xy ? 1 : 0;
  a.n = (uint32_t)n;
  BSMI_HIP(hipMemsetAsync(a.touch, 0, n, s));
  BSMI_HIP(hipMemsetAsync(a.id_keys, 0xff, (cap + 1) * sizeof(uint64_t), s));
  BSMI_HIP(hipMemsetAsync(a.pair_keys, 0xff, cap * sizeof(uint64_t), s));
  BSMI_HIP(hipMemsetAsync(a.pair_counts, 0, cap * sizeof(uint64_t), s));
  BSMI_HIP(hipMemsetAsync(a.flags, 0, 4 * sizeof(uint32_t), s));
  const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 16384);
  const int64_t segs = (int64_t)a.D * a.H * ((a.W + 63) / 64);
  hipLaunchKernelGGL(cc_init_kernel, dim3((unsigned)std::min<int64_t>((segs + 3) / 4, 16384)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(cc_union_kernel, dim3(grid), dim3(256), 0, s, a);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(grid), dim3(256), 0, s, a);
  hipLaunchKernelGGL(fill_count_kernel, dim3(grid), dim3(256), 0, s, a);
  BSMI_HIP(hipGetLastError());

  // the decision, on the host from the read-out table (one entry per enclosed component and neighbouring id: small)
  uint32_t flags[4];
  BSMI_HIP(hipMemcpyAsync(flags, a.flags, sizeof flags, hipMemcpyDeviceToHost, s));
  BSMI_HIP(hipStreamSynchronize(s));
  if (flags[0])
    BSMI_FAIL(BSMI_ERR_OVERFLOW, "fill_holes table overflow (flags 0x%x: 1 face-pair table, 2 id table; capacity %llu)", flags[0],
              (unsigned long long)table_capacity);
  std::vector<uint64_t> roots, fill;
  if (flags[1]) {
    std::vector<uint64_t> ids(cap + 1), keys(cap), counts(cap);
    BSMI_HIP(hipMemcpyAsync(ids.data(), a.id_keys, (cap + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    BSMI_HIP(hipMemcpyAsync(keys.data(), a.pair_keys, cap * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    BSMI_HIP(hipMemcpyAsync(counts.data(), a.pair_counts, cap * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    BSMI_HIP(hipStreamSynchronize(s));
    ids[cap] = kEmpty;
    struct Tally {
      uint64_t total = 0, best = 0, best_id = 0;
    };
    std::unordered_map<uint32_t, Tally> tally;
    for (size_t i = 0; i < cap; ++i) {
      if (keys[i] == kEmpty) continue;
      Tally& t = tally[(uint32_t)(keys[i] >> 32)];
      const uint64_t id = ids[keys[i] & 0xffffffffull], c = counts[i];
      t.total += c;
      if (id != 0 && (c > t.best || (c == t.best && id < t.best_id))) {
        t.best = c;
        t.best_id = id;
      }
    }
    std::vector<std::pair<uint64_t, uint64_t>> chosen;
    for (const auto& kv : tally)
      if (kv.second.best > 0 && BSMI_MORPH_MERGE_DEN * kv.second.best >= BSMI_MORPH_MERGE_NUM * kv.second.total)
        chosen.emplace_back((uint64_t)kv.first, kv.second.best_id);
    std::sort(chosen.begin(), chosen.end());
    for (const auto& c : chosen) {
      roots.push_back(c.first);
      fill.push_back(c.second);
    }
  }
  // the list goes where the tables were (at most one entry per pair-table entry)
  const uint32_t m = (uint32_t)roots.size();
  if (m) {
    BSMI_HIP(hipMemcpyAsync(a.pair_keys, roots.data(), m * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    BSMI_HIP(hipMemcpyAsync(a.pair_counts, fill.data(), m * sizeof(uint64_t), hipMemcpyHostToDevice, s));
  }
  hipLaunchKernelGGL(fill_apply_kernel, dim3(grid), dim3(256), 0, s, a, (const uint64_t*)a.pair_keys, (const uint64_t*)a.pair_counts, m);
  BSMI_HIP(hipGetLastError());
  BSMI_HIP(hipStreamSynchronize(s));  // roots / fill are host vectors of this call
  if (n_filled) *n_filled = m;
  return BSMI_OK;
}

}  // extern "C"

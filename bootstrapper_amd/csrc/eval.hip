// `bs evaluate` on the device (reference evaluate.py:39-101, eval/compute_errors.py, gp/add_aff_errors.py,
// eval/compute_metrics.py).
//
// Affinity errors of a tile of Scan chunks (one layer of chunks, the z range of one chunk across the ROI, or the whole ROI):
//   aff_diff_kernel   diff[v] = sum_e (s_e - p_e)^2 (* mask[v]) in f32 with the reference's rounding, stored as f32 for the
//                     voxels the chunk owns, and the chunk's maximum: a block reduction, then one atomicMax per block on the
//                     bit pattern of the non-negative float
//   aff_norm_kernel   d = diff / max of the owning chunk, error_map = u8(trunc(d * 255)), error_mask = floor < d < ceil, and a
//                     256-bin histogram of error_map plus the count of mask ones (the statistics, exactly, without a read-back)
// Traffic per voxel: seg 8 + K pred + mask 1 + diff 4 written, then diff 4 read + 2 written: 25 B at K = 6 with a mask.
//
// Contingency table of (gt, seg) pairs for Rand / VOI: a tile's distinct gt ids and seg ids get dense ids (their slots in
// two open-addressing tables of 64-bit keys), a pair becomes one 64-bit key (gt slot << 32 | seg slot) in a third table with
// u64 counts.  Runs of equal pairs along x are aggregated within a wave before any atomic.  Counts are exact integers, so the
// table is the same whatever the order of the atomics; the host merges the tiles' triples.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/bsmi.h"
#include "common.h"
#include "u64_table.h"

#include "dev_guard.h"  // last: routes hipMalloc / hipFree through the guarded allocator (BSMI_GUARD_MB)

// the reference evaluates every step in numpy f32: no a*b+c may become one rounding
#pragma clang fp contract(off)

struct bsmi_eval {
  int device = 0;
  uint64_t cap = 0;           // slots of each id table (a power of two; one more slot holds the id 2^64-1) and of the pair table
  uint64_t* gt_keys = nullptr;   // [cap + 1]
  uint64_t* seg_keys = nullptr;  // [cap + 1]
  uint64_t* pair_keys = nullptr; // [cap]
  uint64_t* pair_counts = nullptr;  // [cap]
  uint32_t* flags = nullptr;     // [0]: overflow bits since the last bsmi_eval_status, [1]: pair inserts, [2]: gt, [3]: seg
  float* diff = nullptr;         // affinity errors: f32 diff of a layer
  size_t diff_cap = 0;
  uint32_t* cmax = nullptr;      // per-chunk maxima (float bits)
  size_t cmax_cap = 0;
};

namespace bsmi {
namespace {

constexpr int kMaxOffsets = 16;
constexpr int kRowsPerBlock = 16;

// overflow bits of bsmi_eval::flags[0]
constexpr uint32_t kOvfPairs = 1, kOvfIds = 2, kOvfOut = 4;

struct AffArgs {
  const uint64_t* seg;
  const uint8_t* pred;
  const uint8_t* mask;
  float* diff;
  uint32_t* cmax;
  uint8_t* emap;
  uint8_t* emask;
  unsigned long long* hist;  // [257]
  int tz, ty, tx;            // ROI tile
  int64_t tvox;              // tz * ty * tx
  int sy, sx;                // seg tile row / plane pitch (x extent, y extent)
  int64_t seg_base;          // seg index of tile voxel (0, 0, 0)
  int cz, cy, cx;            // chunk extent (clamped to the tile)
  int ncz, ncy, ncx;         // chunks per axis (the last one snapped to the tile's end)
  int K;
  int64_t delta[kMaxOffsets];  // seg index offset of each neighbour
  float floor_, ceil_;
  int count_z_end;
};

// Scan's chunk that writes a voxel last along one axis: the snapped last chunk covers [n - c, n)
__device__ __forceinline__ int owner(int v, int c, int nc, int n) { return v >= n - c ? nc - 1 : v / c; }

__device__ __forceinline__ float block_max(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  const int w = (threadIdx.y * blockDim.x + threadIdx.x) >> 6;
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float m = red[0];
  for (int i = 1; i < (int)(blockDim.x * blockDim.y) / 64; ++i) m = fmaxf(m, red[i]);
  return m;
}

// grid (blocks per chunk, chunks): a block walks kRowsPerBlock rows (z, y) of its chunk, 64 lanes along x.  KC = the channel
// count when it is known at compile time (the loads of all channels then go out together), 0 = a.K at run time
template <int KC>
__global__ void __launch_bounds__(256) aff_diff_kernel(AffArgs a) {
  __shared__ float red[4];
  const int chunk = blockIdx.y;
  const int jz = chunk / (a.ncy * a.ncx), jyx = chunk - jz * a.ncy * a.ncx;
  const int jy = jyx / a.ncx, jx = jyx - jy * a.ncx;
  const int z0 = jz == a.ncz - 1 ? a.tz - a.cz : jz * a.cz;
  const int y0 = jy == a.ncy - 1 ? a.ty - a.cy : jy * a.cy;
  const int x0 = jx == a.ncx - 1 ? a.tx - a.cx : jx * a.cx;
  const int rows = a.cz * a.cy;
  const float unit = 1.0f / 255.0f;
  float m = 0.0f;
  for (int r = blockIdx.x * kRowsPerBlock + threadIdx.y; r < min(rows, (int)(blockIdx.x + 1) * kRowsPerBlock); r += blockDim.y) {
    const int rz = r / a.cy, z = z0 + rz, y = y0 + (r - rz * a.cy);
    const bool own_zy = owner(z, a.cz, a.ncz, a.tz) == jz && owner(y, a.cy, a.ncy, a.ty) == jy;
    const int64_t vrow = ((int64_t)z * a.ty + y) * a.tx;
    const int64_t srow = a.seg_base + ((int64_t)z * a.sy + y) * a.sx;
    for (int x = x0 + threadIdx.x; x < x0 + a.cx; x += 64) {
      const uint64_t s0 = a.seg[srow + x];
      float diff = 0.0f;
      const int K = KC > 0 ? KC : a.K;
#pragma unroll
      for (int e = 0; e < (KC > 0 ? KC : kMaxOffsets); ++e) {
        if (KC == 0 && e >= K) break;
        const uint64_t s1 = a.seg[srow + x + a.delta[e]];
        const float s = (s0 == s1 && s0 != 0) ? 1.0f : 0.0f;
        const float p = (float)a.pred[e * a.tvox + vrow + x] * unit;
        const float d = s - p;
        diff = diff + d * d;
      }
      if (a.mask) diff = diff * (float)a.mask[vrow + x];
      m = fmaxf(m, diff);
      if (own_zy && owner(x, a.cx, a.ncx, a.tx) == jx) a.diff[vrow + x] = diff;
    }
  }
  m = block_max(m, red);
  if (threadIdx.x == 0 && threadIdx.y == 0 && m > 0.0f) atomicMax(&a.cmax[chunk], __float_as_uint(m));
}

// grid over rows (z, y) of the tile, kRowsPerBlock per block
__global__ void __launch_bounds__(256) aff_norm_kernel(AffArgs a) {
  __shared__ uint32_t hist[257];
  const int tid = threadIdx.y * blockDim.x + threadIdx.x;
  for (int i = tid; i < 257; i += 256) hist[i] = 0;
  __syncthreads();
  const int rows = a.tz * a.ty;
  for (int r = blockIdx.x * kRowsPerBlock + threadIdx.y; r < min(rows, (int)(blockIdx.x + 1) * kRowsPerBlock); r += blockDim.y) {
    const int z = r / a.ty, y = r - z * a.ty;
    const int jzy = owner(z, a.cz, a.ncz, a.tz) * a.ncy + owner(y, a.cy, a.ncy, a.ty);
    const bool counted = z < a.count_z_end;
    const int64_t vrow = (int64_t)r * a.tx;
    for (int x = threadIdx.x; x < a.tx; x += 64) {
      const float m = __uint_as_float(a.cmax[jzy * a.ncx + owner(x, a.cx, a.ncx, a.tx)]);
      const float d = m > 0.0f ? a.diff[vrow + x] / m : 0.0f;
      const uint32_t em = (uint32_t)(d * 255.0f);
      const uint32_t mk = (d > a.floor_ && d < a.ceil_) ? 1u : 0u;
      a.emap[vrow + x] = (uint8_t)em;
      a.emask[vrow + x] = (uint8_t)mk;
      if (counted) {
        atomicAdd(&hist[em], 1u);
        if (mk) atomicAdd(&hist[256], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < 257; i += 256)
    if (hist[i]) atomicAdd(&a.hist[i], (unsigned long long)hist[i]);
}

// ---- contingency table (mix64, table_slot: u64_table.h) ----

struct PairArgs {
  const uint64_t* gt;
  const uint64_t* seg;
  const uint8_t* mask;
  int D, H, W;
  uint64_t cap;
  uint64_t* gt_keys;
  uint64_t* seg_keys;
  uint64_t* pair_keys;
  unsigned long long* pair_counts;
  uint32_t* flags;
};

// an id's dense index: its slot; the id 2^64-1 (the empty marker) has the extra slot `cap`, whose key reads as itself
__device__ __forceinline__ int64_t id_slot(uint64_t* keys, uint64_t cap, uint64_t id, uint32_t* inserts, uint32_t* flags) {
  return id == kEmpty ? (int64_t)cap : table_slot(keys, cap, id, inserts, flags, kOvfIds);
}

// one wave per 64-voxel segment of a row; lanes holding the first voxel of a run of equal (gt, seg) insert the run at once
__global__ void __launch_bounds__(256) pairs_kernel(PairArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t nseg = (a.W + 63) / 64;
  const int64_t items = (int64_t)a.D * a.H * nseg;
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x / 64);
  for (int64_t it = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); it < items; it += nwaves) {
    const int64_t row = it / nseg;
    const int x = (int)(it - row * nseg) * 64 + lane;
    const bool in = x < a.W;
    uint64_t g = 0, s = 0;
    if (in) {
      const int64_t v = row * a.W + x;
      g = a.gt[v];
      s = a.seg[v];
      if (a.mask) {
        const uint64_t m = a.mask[v];
        g *= m;  // the reference multiplies the ids by the mask value, wrapping at 2^64
        s *= m;
      }
    }
    const bool valid = in && g != 0;  // gt 0 is ignored
    const uint64_t pg = __shfl_up(g, 1), ps = __shfl_up(s, 1);
    const int pv = __shfl_up((int)valid, 1);
    const bool head = valid && (lane == 0 || !pv || pg != g || ps != s);
    const uint64_t heads = __ballot(head);
    const uint64_t ends = __ballot(!valid) | heads;  // a run ends at the next head or at the next excluded voxel
    if (head) {
      const uint64_t after = lane == 63 ? 0 : ends & (~0ull << (lane + 1));
      const int next = after ? __ffsll((long long)after) - 1 : 64;
      const int64_t gi = id_slot(a.gt_keys, a.cap, g, a.flags + 2, a.flags);
      const int64_t si = id_slot(a.seg_keys, a.cap, s, a.flags + 3, a.flags);
      if (gi >= 0 && si >= 0) {
        const uint64_t key = (uint64_t)gi << 32 | (uint64_t)si;
        const int64_t p = table_slot(a.pair_keys, a.cap, key, a.flags + 1, a.flags, kOvfPairs);
        if (p >= 0) atomicAdd(&a.pair_counts[p], (unsigned long long)(next - lane));
      }
    }
  }
}

__global__ void pairs_read_kernel(const uint64_t* pair_keys, const uint64_t* pair_counts, const uint64_t* gt_keys,
                                  const uint64_t* seg_keys, uint64_t cap, uint64_t* gt_out, uint64_t* seg_out, uint64_t* count_out,
                                  uint64_t out_cap, unsigned long long* n, uint32_t* flags) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t k = pair_keys[i];
    if (k == kEmpty) continue;
    const unsigned long long j = atomicAdd(n, 1ull);
    if (j >= out_cap) {
      atomicOr(flags, kOvfOut);
      continue;
    }
    gt_out[j] = gt_keys[k >> 32];
    seg_out[j] = seg_keys[k & 0xffffffffull];
    count_out[j] = pair_counts[i];
  }
}

int grow(void** p, size_t* cap, size_t bytes, hipStream_t s) {
  if (*cap >= bytes) return BSMI_OK;
  BSMI_HIP(hipStreamSynchronize(s));
  if (*p) BSMI_HIP(hipFree(*p));
  *p = nullptr;
  *cap = 0;
  BSMI_HIP(hipMalloc(p, bytes));
  *cap = bytes;
  return BSMI_OK;
}

}  // namespace
}  // namespace bsmi

using namespace bsmi;

extern "C" {

int bsmi_eval_create(int device, uint64_t pair_capacity, bsmi_eval** out) {
  if (!out) BSMI_FAIL(BSMI_ERR_INVALID, "null output");
  *out = nullptr;
  if (pair_capacity < 2 || pair_capacity > (1ull << 31) || (pair_capacity & (pair_capacity - 1)))
    BSMI_FAIL(BSMI_ERR_INVALID, "pair_capacity %llu: a power of two in [2, 2^31]", (unsigned long long)pair_capacity);
  BSMI_HIP(hipSetDevice(device));
  bsmi_eval* h = new bsmi_eval();
  h->device = device;
  h->cap = pair_capacity;
  const size_t ids = (pair_capacity + 1) * sizeof(uint64_t), pairs = pair_capacity * sizeof(uint64_t);
  hipError_t e = hipSuccess;
  if (e == hipSuccess) e = hipMalloc(&h->gt_keys, ids);
  if (e == hipSuccess) e = hipMalloc(&h->seg_keys, ids);
  if (e == hipSuccess) e = hipMalloc(&h->pair_keys, pairs);
  if (e == hipSuccess) e = hipMalloc(&h->pair_counts, pairs);
  if (e == hipSuccess) e = hipMalloc(&h->flags, 4 * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemset(h->flags, 0, 4 * sizeof(uint32_t));
  if (e != hipSuccess) {
    bsmi_eval_destroy(h);
    BSMI_FAIL(BSMI_ERR_HIP, "bsmi_eval_create: %s", hipGetErrorString(e));
  }
  *out = h;
  return BSMI_OK;
}

int bsmi_eval_destroy(bsmi_eval* h) {
  if (!h) return BSMI_OK;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  for (void* p : {(void*)h->gt_keys, (void*)h->seg_keys, (void*)h->pair_keys, (void*)h->pair_counts, (void*)h->flags, (void*)h->diff,
                  (void*)h->cmax})
    if (p) (void)hipFree(p);
  delete h;
  return BSMI_OK;
}

int bsmi_eval_aff_errors_u8(bsmi_eval* h, const uint64_t* seg_dev, const int64_t seg_shape[3], const int64_t seg_origin[3],
                            const uint8_t* pred_dev, int n_channels, const int64_t tile_shape[3], const uint8_t* mask_dev,
                            const int32_t* offsets, const int64_t chunk_shape[3], float floor_, float ceil_, int64_t count_z_end,
                            uint8_t* error_map_dev, uint8_t* error_mask_dev, uint64_t* hist_dev, void* stream) {
  if (!h || !seg_dev || !seg_shape || !seg_origin || !pred_dev || !tile_shape || !offsets || !chunk_shape || !error_map_dev ||
      !error_mask_dev || !hist_dev)
    BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (n_channels < 1 || n_channels > kMaxOffsets) BSMI_FAIL(BSMI_ERR_INVALID, "n_channels %d: 1..%d", n_channels, kMaxOffsets);
  for (int d = 0; d < 3; ++d)
    if (tile_shape[d] < 1 || tile_shape[d] > (1 << 20) || seg_shape[d] < 1)
      BSMI_FAIL(BSMI_ERR_INVALID, "tile / seg shape out of range on axis %d", d);
  const int64_t tvox = tile_shape[0] * tile_shape[1] * tile_shape[2];
  if (tile_shape[0] * tile_shape[1] >= (1ll << 31) || tvox * n_channels >= (1ll << 40))
    BSMI_FAIL(BSMI_ERR_INVALID, "tile too large");
  // every neighbour of every tile voxel must lie in the seg tile (the caller reads the halo, zeros beyond the dataset)
  for (int e = 0; e < n_channels; ++e)
    for (int d = 0; d < 3; ++d) {
      const int64_t o = offsets[3 * e + d];
      if (seg_origin[d] > std::min<int64_t>(0, o) || seg_origin[d] + seg_shape[d] < tile_shape[d] + std::max<int64_t>(0, o))
        BSMI_FAIL(BSMI_ERR_INVALID, "offset %d (%lld) on axis %d leaves the seg tile (origin %lld, extent %lld, tile %lld)", e,
                  (long long)o, d, (long long)seg_origin[d], (long long)seg_shape[d], (long long)tile_shape[d]);
    }
  if (chunk_shape[0] < 1 || chunk_shape[1] < 1 || chunk_shape[2] < 1) BSMI_FAIL(BSMI_ERR_INVALID, "chunk extent must be positive");
  if (count_z_end < 0 || count_z_end > tile_shape[0]) BSMI_FAIL(BSMI_ERR_INVALID, "count_z_end outside the tile");
  BSMI_HIP(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  AffArgs a{};
  a.tz = (int)tile_shape[0];
  a.ty = (int)tile_shape[1];
  a.tx = (int)tile_shape[2];
  a.tvox = tvox;
  a.sy = (int)seg_shape[1];
  a.sx = (int)seg_shape[2];
  a.seg_base = ((-seg_origin[0]) * seg_shape[1] + (-seg_origin[1])) * seg_shape[2] + (-seg_origin[2]);
  a.cz = (int)std::min<int64_t>(chunk_shape[0], a.tz);
  a.cy = (int)std::min<int64_t>(chunk_shape[1], a.ty);
  a.cx = (int)std::min<int64_t>(chunk_shape[2], a.tx);
  a.ncz = ceil_div(a.tz, a.cz);
  a.ncy = ceil_div(a.ty, a.cy);
  a.ncx = ceil_div(a.tx, a.cx);
  if ((int64_t)a.ncz * a.ncy * a.ncx > 65535) BSMI_FAIL(BSMI_ERR_INVALID, "more than 65535 chunks in one tile");
  a.K = n_channels;
  for (int e = 0; e < n_channels; ++e)
    a.delta[e] = ((int64_t)offsets[3 * e] * seg_shape[1] + offsets[3 * e + 1]) * seg_shape[2] + offsets[3 * e + 2];
  a.floor_ = floor_;
  a.ceil_ = ceil_;
  a.count_z_end = (int)count_z_end;
  a.seg = seg_dev;
  a.pred = pred_dev;
  a.mask = mask_dev;
  a.emap = error_map_dev;
  a.emask = error_mask_dev;
  a.hist = (unsigned long long*)hist_dev;
  const int nch = a.ncz * a.ncy * a.ncx;
  int rc = grow((void**)&h->diff, &h->diff_cap, (size_t)tvox * sizeof(float), s);
  if (rc) return rc;
  rc = grow((void**)&h->cmax, &h->cmax_cap, (size_t)nch * sizeof(uint32_t), s);
  if (rc) return rc;
  a.diff = h->diff;
  a.cmax = h->cmax;
  BSMI_HIP(hipMemsetAsync(h->cmax, 0, (size_t)nch * sizeof(uint32_t), s));
  const dim3 blk(64, 4);
  const dim3 grid((unsigned)ceil_div(a.cz * a.cy, kRowsPerBlock), (unsigned)nch);
  if (a.K == 6)
    hipLaunchKernelGGL(aff_diff_kernel<6>, grid, blk, 0, s, a);
  else if (a.K == 3)
    hipLaunchKernelGGL(aff_diff_kernel<3>, grid, blk, 0, s, a);
  else
    hipLaunchKernelGGL(aff_diff_kernel<0>, grid, blk, 0, s, a);
  hipLaunchKernelGGL(aff_norm_kernel, dim3((unsigned)ceil_div(a.tz * a.ty, kRowsPerBlock)), blk, 0, s, a);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_eval_pairs_u64(bsmi_eval* h, const uint64_t* gt_dev, const uint64_t* seg_dev, const uint8_t* mask_dev, const int64_t shape[3],
                        int reset, void* stream) {
  if (!h || !gt_dev || !seg_dev || !shape) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  for (int d = 0; d < 3; ++d)
    if (shape[d] < 0 || shape[d] > (1 << 30)) BSMI_FAIL(BSMI_ERR_INVALID, "shape out of range on axis %d", d);
  BSMI_HIP(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  if (reset) {
    BSMI_HIP(hipMemsetAsync(h->gt_keys, 0xff, (h->cap + 1) * sizeof(uint64_t), s));
    BSMI_HIP(hipMemsetAsync(h->seg_keys, 0xff, (h->cap + 1) * sizeof(uint64_t), s));
    BSMI_HIP(hipMemsetAsync(h->pair_keys, 0xff, h->cap * sizeof(uint64_t), s));
    BSMI_HIP(hipMemsetAsync(h->pair_counts, 0, h->cap * sizeof(uint64_t), s));
    BSMI_HIP(hipMemsetAsync(h->flags + 1, 0, 3 * sizeof(uint32_t), s));
  }
  const int64_t items = shape[0] * shape[1] * ((shape[2] + 63) / 64);
  if (items == 0) return BSMI_OK;
  PairArgs a{gt_dev, seg_dev, mask_dev, (int)shape[0], (int)shape[1], (int)shape[2], h->cap, h->gt_keys, h->seg_keys,
             h->pair_keys, (unsigned long long*)h->pair_counts, h->flags};
  const unsigned blocks = (unsigned)std::min<int64_t>((items + 3) / 4, 16384);
  hipLaunchKernelGGL(pairs_kernel, dim3(blocks), dim3(256), 0, s, a);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_eval_pairs_read(bsmi_eval* h, uint64_t* gt_out_dev, uint64_t* seg_out_dev, uint64_t* count_out_dev, uint64_t out_capacity,
                         uint64_t* n_dev, void* stream) {
  if (!h || !gt_out_dev || !seg_out_dev || !count_out_dev || !n_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  BSMI_HIP(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  BSMI_HIP(hipMemsetAsync(n_dev, 0, sizeof(uint64_t), s));
  const unsigned blocks = (unsigned)std::min<uint64_t>((h->cap + 255) / 256, 4096);
  hipLaunchKernelGGL(pairs_read_kernel, dim3(blocks), dim3(256), 0, s, h->pair_keys, h->pair_counts, h->gt_keys, h->seg_keys, h->cap,
                     gt_out_dev, seg_out_dev, count_out_dev, out_capacity, (unsigned long long*)n_dev, h->flags);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_eval_status(bsmi_eval* h, void* stream) {
  if (!h) BSMI_FAIL(BSMI_ERR_INVALID, "null handle");
  BSMI_HIP(hipSetDevice(h->device));
  uint32_t f[4];
  BSMI_HIP(hipMemcpyAsync(f, h->flags, sizeof f, hipMemcpyDeviceToHost, (hipStream_t)stream));
  BSMI_HIP(hipStreamSynchronize((hipStream_t)stream));
  if (f[0]) {
    BSMI_HIP(hipMemsetAsync(h->flags, 0, sizeof(uint32_t), (hipStream_t)stream));
    BSMI_HIP(hipStreamSynchronize((hipStream_t)stream));
    BSMI_FAIL(BSMI_ERR_OVERFLOW, "evaluation table overflow (flags 0x%x: 1 pair table, 2 id tables, 4 read-out buffer; capacity %llu)", f[0],
              (unsigned long long)h->cap);
  }
  return BSMI_OK;
}

}  // extern "C"

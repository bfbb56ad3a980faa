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
// LSD errors of a tile of Scan chunks (gp/add_lsd_errors.py; `bsmi_eval_lsd_errors_u8`): see "LSD errors" below.
//
// Contingency table of (gt, seg) pairs for Rand / VOI: a tile's distinct gt ids and seg ids get dense ids (their slots in
// two open-addressing tables of 64-bit keys), a pair becomes one 64-bit key (gt slot << 32 | seg slot) in a third table with
// u64 counts.  Runs of equal pairs along x are aggregated within a wave before any atomic.  Counts are exact integers, so the
// table is the same whatever the order of the atomics; the host merges the tiles' triples.
#include <hip/hip_runtime.h>

#include <cmath>
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
  // LSD errors: scratch of one group of chunks, the id table that makes labels 32-bit, the window weights
  void* lsd_scratch = nullptr;
  size_t lsd_scratch_cap = 0;
  uint64_t* lsd_keys = nullptr;  // [cap + 1]
  size_t lsd_keys_cap = 0;
  uint32_t* lsd_inserts = nullptr;
  double* lsd_w = nullptr;       // 3 tables (w, w c, w c^2) per axis
  size_t lsd_w_cap = 0;
  float lsd_w_key[7] = {0, 0, 0, 0, 0, 0, 0};  // sigma, voxel_size, downsample of the tables held
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

// ---- LSD errors (gp/add_lsd_errors.py) ---------------------------------------------------------------------------------
// Per Scan chunk the reference works on the chunk grown by a margin (region G): descriptors of the segmentation over G from
// the label array L = G grown by the context, diff against pred, one maximum over G, threshold, morphology over G, and only
// then the crop to the chunk.  The kernels below run on a group of chunks at a time (grid y = the chunk within the group):
//   lsd_sub_kernel    sub[c] = 32-bit id (slot + 1 in an id table) of L[::df], 0 for background
//   lsd_desc_kernel   one thread per cell of the sub-grid: the Gaussian-window statistics once per (cell, label), shared by the
//                     cell's df^3 voxels; the sub-grid window of a block of 2 x 8 x 16 cells is staged in LDS.  Along x a tap
//                     costs one LDS read, one compare and one bit: six taps make an index into a table of their partial sums
//                     (sum w, sum w c, sum w c^2 of the taps whose bit is set), so float64 work is three adds per six taps;
//                     the row sums are folded into the y and z moments.  The diff against pred is fused in; the per-chunk
//                     maximum is a block reduction and one atomicMax per block
//   lsd_norm_kernel   d = diff / max, the raw mask over G, error_map and its histogram for the voxels the chunk owns
//   lsd_xy_kernel     in-plane erosion / dilation by the L1 diamond of radius 4 (= 4 iterations of the 4-neighbour cross), 0 outside G
//   lsd_zclose_kernel z closing by the 3-column with 0 outside G, cropped to the chunk; error_mask and the count of its ones
constexpr int kLsdBZ = 2, kLsdBY = 8, kLsdBX = 16;  // cells of one block of lsd_desc_kernel
constexpr size_t kLsdLdsBytes = 72704;              // tables + window of one block: with the item list, two blocks to a CU
constexpr int kLsdMaxDownsample = 2;
constexpr int kLsdMaxItems = 256 * kLsdMaxDownsample * kLsdMaxDownsample * kLsdMaxDownsample;  // (cell, label) pairs of a block
constexpr int kLsdTapBits = 6;                      // taps along x per table lookup
constexpr int kLsdWinPad = 8;                       // cells after the window that the last group of the last row may read
constexpr uint32_t kLsdNoId = 0xffffffffu;          // a label that is nowhere on the sub-grid
constexpr int kLsdMorphRadius = 4;

struct LsdArgs {
  const uint64_t* seg;
  const uint8_t* pred;
  const uint8_t* mask;
  int tz, ty, tx;           // ROI tile
  int cz, cy, cx;           // chunk extent (clamped to the tile)
  int ncz, ncy, ncx;        // chunks per axis
  int mz, my, mx;           // margin
  int kz, ky, kx;           // context of the label array
  int gz, gy, gx;           // G = chunk + 2 margin
  int sd, sh, sw;           // sub-grid extent: (G + 2 context) / df
  int df;
  int rz, ry, rx;           // window radii on the sub-grid
  int64_t gvox, svox;       // voxels of G, cells of the sub-grid
  int sy, sx;               // seg tile: y extent, x extent
  int64_t seg_base;         // seg index of tile voxel (0, 0, 0)
  int py, px;               // pred / mask tile (tile + 2 margin): y extent, x extent
  int64_t pvox;             // its voxels
  float sigma[3];
  float step[3];            // world distance between sub-grid points
  uint32_t* sub;            // [group][svox]
  float* diff;              // [group][gvox]
  uint8_t* raw;             // [group][gvox] thresholded mask
  uint8_t* e1;              // [group][gvox] eroded
  uint8_t* e2;              // [group][gvox] opened
  uint32_t* cmax;           // [chunks of the tile]
  int chunk0;               // first chunk of the group
  float* dbg_desc;          // [chunks][10][gvox] or null
  const double* w;          // window tables: z and y: w[2r+1], w c[2r+1], w c^2[2r+1]; x: [groups][64][3] partial sums of the same
  uint64_t* keys;
  uint64_t cap;
  uint32_t* inserts;
  uint32_t* flags;
  uint8_t* emap;
  uint8_t* emask;
  unsigned long long* hist;
  float floor_, ceil_;
  int count_z_end;
};

struct ChunkAt {
  int jz, jy, jx, z0, y0, x0;
};

__device__ __forceinline__ ChunkAt lsd_chunk(const LsdArgs& a, int chunk) {
  ChunkAt c;
  c.jz = chunk / (a.ncy * a.ncx);
  const int jyx = chunk - c.jz * a.ncy * a.ncx;
  c.jy = jyx / a.ncx;
  c.jx = jyx - c.jy * a.ncx;
  c.z0 = c.jz == a.ncz - 1 ? a.tz - a.cz : c.jz * a.cz;
  c.y0 = c.jy == a.ncy - 1 ? a.ty - a.cy : c.jy * a.cy;
  c.x0 = c.jx == a.ncx - 1 ? a.tx - a.cx : c.jx * a.cx;
  return c;
}

// seg index of voxel (z, y, x) of chunk c's region G
__device__ __forceinline__ int64_t lsd_seg_index(const LsdArgs& a, const ChunkAt& c, int z, int y, int x) {
  return a.seg_base + ((int64_t)(c.z0 - a.mz + z) * a.sy + (c.y0 - a.my + y)) * a.sx + (c.x0 - a.mx + x);
}

__device__ __forceinline__ uint32_t lsd_find(const uint64_t* keys, uint64_t cap, uint64_t key) {
  if (key == kEmpty) return (uint32_t)cap + 1;
  uint64_t h = mix64(key) & (cap - 1);
  for (uint64_t probe = 0; probe < cap; ++probe) {
    const uint64_t k = keys[h];
    if (k == key) return (uint32_t)h + 1;
    if (k == kEmpty) return kLsdNoId;
    h = (h + 1) & (cap - 1);
  }
  return kLsdNoId;
}

__global__ void __launch_bounds__(256) lsd_sub_kernel(LsdArgs a) {
  const ChunkAt c = lsd_chunk(a, a.chunk0 + blockIdx.y);
  uint32_t* sub = a.sub + (int64_t)blockIdx.y * a.svox;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.svox; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % a.sw), y = (int)((i / a.sw) % a.sh), z = (int)(i / ((int64_t)a.sw * a.sh));
    const uint64_t l = a.seg[lsd_seg_index(a, c, z * a.df - a.kz, y * a.df - a.ky, x * a.df - a.kx)];
    uint32_t id = 0;
    if (l != 0) {
      const int64_t slot = id_slot(a.keys, a.cap, l, a.inserts, a.flags);
      id = slot < 0 ? kLsdNoId : (uint32_t)slot + 1;
    }
    sub[i] = id;
  }
}

__global__ void __launch_bounds__(256) lsd_desc_kernel(LsdArgs a) {
  extern __shared__ double lsd_lds[];
  __shared__ float red[4];
  __shared__ uint32_t items[kLsdMaxItems];
  __shared__ uint32_t n_items[2];
  const int nz = 2 * a.rz + 1, ny = 2 * a.ry + 1, nx = 2 * a.rx + 1;
  const int ngroups = (nx + kLsdTapBits - 1) / kLsdTapBits;
  const uint32_t last_bits = (1u << (nx - (ngroups - 1) * kLsdTapBits)) - 1;  // the last group's taps inside the window
  const int ntab = 3 * (nz + ny) + ngroups * (3 << kLsdTapBits);
  double* tab = lsd_lds;
  uint32_t* win = (uint32_t*)(tab + ntab);
  const double *tz0 = tab, *tz1 = tab + nz, *tz2 = tab + 2 * nz;
  const double *ty0 = tab + 3 * nz, *ty1 = ty0 + ny, *ty2 = ty0 + 2 * ny;
  const double* tx = ty0 + 3 * ny;
  const int tid = threadIdx.x;
  const int slot = blockIdx.y, chunk = a.chunk0 + slot;
  const ChunkAt c = lsd_chunk(a, chunk);
  const int df = a.df;
  const int ncz = a.gz / df, ncy = a.gy / df, ncx = a.gx / df;  // cells of G
  const int nbx = (ncx + kLsdBX - 1) / kLsdBX, nby = (ncy + kLsdBY - 1) / kLsdBY;
  const int bx = blockIdx.x % nbx, by = (blockIdx.x / nbx) % nby, bz = blockIdx.x / (nbx * nby);
  const int c0z = bz * kLsdBZ, c0y = by * kLsdBY, c0x = bx * kLsdBX;  // first cell of the block, in cells of G
  const int ez = kLsdBZ + 2 * a.rz, ey = kLsdBY + 2 * a.ry, ex = kLsdBX + 2 * a.rx;  // window extent
  if (tid < 2) n_items[tid] = 0;
  for (int i = tid; i < ntab; i += 256) tab[i] = a.w[i];
  {
    // the window's first cell on the sub-grid: G's first cell is context / df
    const int wz = a.kz / df + c0z - a.rz, wy = a.ky / df + c0y - a.ry, wx = a.kx / df + c0x - a.rx;
    const uint32_t* sub = a.sub + (int64_t)slot * a.svox;
    for (int i = tid; i < ez * ey * ex + kLsdWinPad; i += 256) {
      const int x = i % ex, y = (i / ex) % ey, z = i / (ex * ey);
      const int X = wx + x, Y = wy + y, Z = wz + z;
      const bool in = z < ez && X >= 0 && X < a.sw && Y >= 0 && Y < a.sh && Z >= 0 && Z < a.sd;
      win[i] = in ? sub[((int64_t)Z * a.sh + Y) * a.sw + X] : 0u;
    }
  }
  __syncthreads();
  // the work items of the block: one per (cell, label), named by the cell and the first voxel of the cell with that label.
  // Objects go to the front of the list and background to its back, so that the lanes of a pass have the same work; a cell
  // that straddles several objects then costs the block its share of passes, not every lane of its wave a whole sweep
  const int nvox = df * df * df;
  {
    const int lx = tid % kLsdBX, ly = (tid / kLsdBX) % kLsdBY, lz = tid / (kLsdBX * kLsdBY);
    const int cellz = c0z + lz, celly = c0y + ly, cellx = c0x + lx;
    if (cellz < ncz && celly < ncy && cellx < ncx)
      for (int k = 0; k < nvox; ++k) {
        const uint64_t l = a.seg[lsd_seg_index(a, c, cellz * df + k / (df * df), celly * df + (k / df) % df, cellx * df + k % df)];
        bool first = true;
        for (int j = 0; j < k; ++j)
          if (a.seg[lsd_seg_index(a, c, cellz * df + j / (df * df), celly * df + (j / df) % df, cellx * df + j % df)] == l) first = false;
        if (!first) continue;
        const uint32_t item = (uint32_t)tid << 3 | (uint32_t)k;
        if (l != 0)
          items[atomicAdd(&n_items[0], 1u)] = item;
        else
          items[kLsdMaxItems - 1 - atomicAdd(&n_items[1], 1u)] = item;
      }
  }
  __syncthreads();
  const int n_obj = (int)n_items[0], n_all = n_obj + (int)n_items[1];
  float bmax = 0.0f;
  {
    const float unit = 1.0f / 255.0f;
    for (int it = tid; it < n_all; it += 256) {
      const uint32_t item = items[it < n_obj ? it : kLsdMaxItems - 1 - (it - n_obj)];
      const int cell = (int)(item >> 3), k = (int)(item & 7);
      const int lx = cell % kLsdBX, ly = (cell / kLsdBX) % kLsdBY, lz = cell / (kLsdBX * kLsdBY);
      const int cellz = c0z + lz, celly = c0y + ly, cellx = c0x + lx;
      const uint32_t* wbase = win + ((int64_t)lz * ey + ly) * ex + lx;
      const uint64_t l = a.seg[lsd_seg_index(a, c, cellz * df + k / (df * df), celly * df + (k / df) % df, cellx * df + k % df)];
      float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f, o4 = 0.f, o5 = 0.f, o6 = 0.f, o7 = 0.f, o8 = 0.f, o9 = 0.f;
      if (l != 0) {
        const uint32_t id = lsd_find(a.keys, a.cap, l);
        double n = 0, m0 = 0, m1 = 0, m2 = 0, c00 = 0, c11 = 0, c22 = 0, c01 = 0, c02 = 0, c12 = 0;
        for (int dz = 0; dz < nz; ++dz) {
          double p0 = 0, p1x = 0, p2x = 0, p1y = 0, p2y = 0, pyx = 0;
          for (int dy = 0; dy < ny; ++dy) {
            const uint32_t* row = wbase + ((int64_t)dz * ey + dy) * ex;
            double s0 = 0, s1 = 0, s2 = 0;
            for (int g = 0; g < ngroups; ++g) {
              // the last group reads up to 5 cells past the lane's taps (the row's other cells, the next row, the pad): masked
              uint32_t bits = 0;
#pragma unroll
              for (int b = 0; b < kLsdTapBits; ++b) bits |= (row[g * kLsdTapBits + b] == id ? 1u : 0u) << b;
              if (g == ngroups - 1) bits &= last_bits;
              if (bits) {
                const double* t = tx + ((g << kLsdTapBits) + bits) * 3;
                s0 += t[0];
                s1 += t[1];
                s2 += t[2];
              }
            }
            const double g0 = ty0[dy], g1 = ty1[dy], g2 = ty2[dy];
            p0 += g0 * s0;
            p1x += g0 * s1;
            p2x += g0 * s2;
            p1y += g1 * s0;
            p2y += g2 * s0;
            pyx += g1 * s1;
          }
          const double h0 = tz0[dz], h1 = tz1[dz], h2 = tz2[dz];
          n += h0 * p0;
          m0 += h1 * p0;
          m1 += h0 * p1y;
          m2 += h0 * p1x;
          c00 += h2 * p0;
          c11 += h0 * p2y;
          c22 += h0 * p2x;
          c01 += h1 * p1y;
          c02 += h1 * p1x;
          c12 += h0 * pyx;
        }
        // a label that no tap of the window holds (a thin object between the sub-grid's points): the library divides by 1
        // instead of the count, so its mean is the ABSOLUTE coordinate 0 of the label array and its covariance 0
        const bool none = n == 0;
        const double cnt = none ? 1.0 : n;
        const double e0 = none ? -(double)(a.kz / df + cellz) * a.step[0] : m0 / cnt;
        const double e1 = none ? -(double)(a.ky / df + celly) * a.step[1] : m1 / cnt;
        const double e2 = none ? -(double)(a.kx / df + cellx) * a.step[2] : m2 / cnt;
        double v0 = none ? 0.0 : c00 / cnt - e0 * e0, v1 = none ? 0.0 : c11 / cnt - e1 * e1, v2 = none ? 0.0 : c22 / cnt - e2 * e2;
        double q0 = none ? 0.0 : c01 / cnt - e0 * e1, q1 = none ? 0.0 : c02 / cnt - e0 * e2, q2 = none ? 0.0 : c12 / cnt - e1 * e2;
        v0 = v0 < 1e-3 ? 1e-3 : v0;
        v1 = v1 < 1e-3 ? 1e-3 : v1;
        v2 = v2 < 1e-3 ? 1e-3 : v2;
        q0 /= sqrt(v0 * v1);
        q1 /= sqrt(v0 * v2);
        q2 /= sqrt(v1 * v2);
        const double g0 = a.sigma[0], g1 = a.sigma[1], g2 = a.sigma[2];
        o0 = (float)(e0 / g0 * 0.5 + 0.5);
        o1 = (float)(e1 / g1 * 0.5 + 0.5);
        o2 = (float)(e2 / g2 * 0.5 + 0.5);
        o3 = (float)(v0 / (g0 * g0));
        o4 = (float)(v1 / (g1 * g1));
        o5 = (float)(v2 / (g2 * g2));
        o6 = (float)(q0 * 0.5 + 0.5);
        o7 = (float)(q1 * 0.5 + 0.5);
        o8 = (float)(q2 * 0.5 + 0.5);
        o9 = (float)n;
#define BSMI_CLIP01(v) v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v)
        BSMI_CLIP01(o0); BSMI_CLIP01(o1); BSMI_CLIP01(o2); BSMI_CLIP01(o3); BSMI_CLIP01(o4);
        BSMI_CLIP01(o5); BSMI_CLIP01(o6); BSMI_CLIP01(o7); BSMI_CLIP01(o8); BSMI_CLIP01(o9);
#undef BSMI_CLIP01
      }
      // every voxel of the cell with this label: the diff against pred, in numpy's order (channels summed one after another)
      for (int j = k; j < nvox; ++j) {
        const int vz = cellz * df + j / (df * df), vy = celly * df + (j / df) % df, vx = cellx * df + j % df;
        if (a.seg[lsd_seg_index(a, c, vz, vy, vx)] != l) continue;
        const int64_t gi = ((int64_t)vz * a.gy + vy) * a.gx + vx;
        const int64_t pi = ((int64_t)(c.z0 + vz) * a.py + (c.y0 + vy)) * a.px + (c.x0 + vx);  // tile + margin coordinates
        const uint8_t* p = a.pred + pi;
        float d, diff;
#define BSMI_TERM(o, ch) d = o - (float)p[(int64_t)(ch) * a.pvox] * unit
        BSMI_TERM(o0, 0); diff = d * d;
        BSMI_TERM(o1, 1); diff = diff + d * d;
        BSMI_TERM(o2, 2); diff = diff + d * d;
        BSMI_TERM(o3, 3); diff = diff + d * d;
        BSMI_TERM(o4, 4); diff = diff + d * d;
        BSMI_TERM(o5, 5); diff = diff + d * d;
        BSMI_TERM(o6, 6); diff = diff + d * d;
        BSMI_TERM(o7, 7); diff = diff + d * d;
        BSMI_TERM(o8, 8); diff = diff + d * d;
        BSMI_TERM(o9, 9); diff = diff + d * d;
#undef BSMI_TERM
        if (a.mask) diff = diff * (float)a.mask[pi];
        bmax = fmaxf(bmax, diff);
        a.diff[(int64_t)slot * a.gvox + gi] = diff;
        if (a.dbg_desc) {
          float* o = a.dbg_desc + (int64_t)chunk * 10 * a.gvox + gi;
          o[0] = o0; o[a.gvox] = o1; o[2 * a.gvox] = o2; o[3 * a.gvox] = o3; o[4 * a.gvox] = o4;
          o[5 * a.gvox] = o5; o[6 * a.gvox] = o6; o[7 * a.gvox] = o7; o[8 * a.gvox] = o8; o[9 * a.gvox] = o9;
        }
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) bmax = fmaxf(bmax, __shfl_xor(bmax, o));
  if ((tid & 63) == 0) red[tid >> 6] = bmax;
  __syncthreads();
  if (tid == 0) {
    const float m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (m > 0.0f) atomicMax(&a.cmax[chunk], __float_as_uint(m));
  }
}

// grid (rows of G / kRowsPerBlock, chunks of the group), block (64, 4)
__global__ void __launch_bounds__(256) lsd_norm_kernel(LsdArgs a) {
  __shared__ uint32_t hist[256];
  const int tid = threadIdx.y * blockDim.x + threadIdx.x;
  hist[tid] = 0;
  __syncthreads();
  const int slot = blockIdx.y, chunk = a.chunk0 + slot;
  const ChunkAt c = lsd_chunk(a, chunk);
  const float m = __uint_as_float(a.cmax[chunk]);
  const int rows = a.gz * a.gy;
  for (int r = blockIdx.x * kRowsPerBlock + threadIdx.y; r < min(rows, (int)(blockIdx.x + 1) * kRowsPerBlock); r += blockDim.y) {
    const int vz = r / a.gy, vy = r - vz * a.gy;
    const int qz = vz - a.mz, qy = vy - a.my;  // chunk coordinates
    const int tz_ = c.z0 + qz, ty_ = c.y0 + qy;
    const bool own_zy = qz >= 0 && qz < a.cz && qy >= 0 && qy < a.cy && owner(tz_, a.cz, a.ncz, a.tz) == c.jz &&
                        owner(ty_, a.cy, a.ncy, a.ty) == c.jy;
    const int64_t grow_ = (int64_t)slot * a.gvox + (int64_t)r * a.gx;
    for (int vx = threadIdx.x; vx < a.gx; vx += 64) {
      const float d = m > 0.0f ? a.diff[grow_ + vx] / m : 0.0f;
      a.raw[grow_ + vx] = (d > a.floor_ && d < a.ceil_) ? 1 : 0;
      const int qx = vx - a.mx, tx_ = c.x0 + qx;
      if (own_zy && qx >= 0 && qx < a.cx && owner(tx_, a.cx, a.ncx, a.tx) == c.jx) {
        const uint32_t em = (uint32_t)(d * 255.0f);
        a.emap[((int64_t)tz_ * a.ty + ty_) * a.tx + tx_] = (uint8_t)em;
        if (tz_ < a.count_z_end) atomicAdd(&hist[em], 1u);
      }
    }
  }
  __syncthreads();
  if (hist[tid]) atomicAdd(&a.hist[tid], (unsigned long long)hist[tid]);
}

// in-plane erosion (ERODE) or dilation by the diamond |dy| + |dx| <= 4 inside G, 0 outside; same grid as lsd_norm_kernel
template <bool ERODE>
__global__ void __launch_bounds__(256) lsd_xy_kernel(LsdArgs a, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst) {
  const int rows = a.gz * a.gy;
  constexpr int R = kLsdMorphRadius;
  for (int r = blockIdx.x * kRowsPerBlock + threadIdx.y; r < min(rows, (int)(blockIdx.x + 1) * kRowsPerBlock); r += blockDim.y) {
    const int vy = r % a.gy;
    const int64_t row = (int64_t)blockIdx.y * a.gvox + (int64_t)r * a.gx;
    for (int vx = threadIdx.x; vx < a.gx; vx += 64) {
      bool v;
      if (ERODE) {
        v = src[row + vx] && vy >= R && vy < a.gy - R && vx >= R && vx < a.gx - R;
        if (v)
          for (int dy = -R; dy <= R; ++dy) {
            const int w = R - (dy < 0 ? -dy : dy);
            for (int dx = -w; dx <= w; ++dx) v = v && src[row + (int64_t)dy * a.gx + vx + dx];
          }
      } else {
        v = false;
        for (int dy = -R; dy <= R; ++dy) {
          if (vy + dy < 0 || vy + dy >= a.gy) continue;
          const int w = R - (dy < 0 ? -dy : dy);
          for (int dx = max(-w, -vx); dx <= min(w, a.gx - 1 - vx); ++dx) v = v || src[row + (int64_t)dy * a.gx + vx + dx];
        }
      }
      dst[row + vx] = v ? 1 : 0;
    }
  }
}

// grid (rows of the chunk / kRowsPerBlock, chunks of the group), block (64, 4)
__global__ void __launch_bounds__(256) lsd_zclose_kernel(LsdArgs a) {
  __shared__ uint32_t ones;
  const int tid = threadIdx.y * blockDim.x + threadIdx.x;
  if (tid == 0) ones = 0;
  __syncthreads();
  const ChunkAt c = lsd_chunk(a, a.chunk0 + blockIdx.y);
  const uint8_t* e2 = a.e2 + (int64_t)blockIdx.y * a.gvox;
  const int64_t plane = (int64_t)a.gy * a.gx;
  const int rows = a.cz * a.cy;
  uint32_t mine = 0;
  for (int r = blockIdx.x * kRowsPerBlock + threadIdx.y; r < min(rows, (int)(blockIdx.x + 1) * kRowsPerBlock); r += blockDim.y) {
    const int qz = r / a.cy, qy = r - qz * a.cy;
    const int tz_ = c.z0 + qz, ty_ = c.y0 + qy;
    if (owner(tz_, a.cz, a.ncz, a.tz) != c.jz || owner(ty_, a.cy, a.ncy, a.ty) != c.jy) continue;
    const int vz = qz + a.mz;
    for (int qx = threadIdx.x; qx < a.cx; qx += 64) {
      const int tx_ = c.x0 + qx;
      if (owner(tx_, a.cx, a.ncx, a.tx) != c.jx) continue;
      const int64_t gi = ((int64_t)vz * a.gy + (qy + a.my)) * a.gx + (qx + a.mx);
      // e[i] = opened mask at vz - 2 + i, 0 outside G; dilation then erosion by the 3-column, both with 0 beyond G
      bool v = vz >= 1 && vz < a.gz - 1;
      if (v) {
        const bool e0 = vz >= 2 && e2[gi - 2 * plane], e1 = e2[gi - plane], ec = e2[gi], e3 = e2[gi + plane];
        const bool e4 = vz < a.gz - 2 && e2[gi + 2 * plane];
        v = (e0 || e1 || ec) && (e1 || ec || e3) && (ec || e3 || e4);
      }
      a.emask[((int64_t)tz_ * a.ty + ty_) * a.tx + tx_] = v ? 1 : 0;
      if (v && tz_ < a.count_z_end) ++mine;
    }
  }
  if (mine) atomicAdd(&ones, mine);
  __syncthreads();
  if (tid == 0 && ones) atomicAdd(&a.hist[256], (unsigned long long)ones);
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
                  (void*)h->cmax, h->lsd_scratch, (void*)h->lsd_keys, (void*)h->lsd_inserts, (void*)h->lsd_w})
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

int bsmi_eval_lsd_errors_u8(bsmi_eval* h, const uint64_t* seg_dev, const int64_t seg_shape[3], const int64_t seg_origin[3],
                            const uint8_t* pred_dev, const uint8_t* mask_dev, const int64_t tile_shape[3], const int64_t chunk_shape[3],
                            const int64_t margin[3], const int64_t context[3], const float sigma[3], const float voxel_size[3],
                            int downsample, float floor_, float ceil_, int64_t count_z_end, uint64_t scratch_limit_bytes,
                            uint8_t* error_map_dev, uint8_t* error_mask_dev, uint64_t* hist_dev, float* debug_desc_dev,
                            float* debug_diff_dev, float* debug_max_dev, uint8_t* debug_raw_mask_dev, void* stream) {
  if (!h || !seg_dev || !seg_shape || !seg_origin || !pred_dev || !tile_shape || !chunk_shape || !margin || !context || !sigma ||
      !voxel_size || !error_map_dev || !error_mask_dev || !hist_dev)
    BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (downsample < 1 || downsample > kLsdMaxDownsample) BSMI_FAIL(BSMI_ERR_INVALID, "downsample %d outside 1..%d", downsample, kLsdMaxDownsample);
  const int df = downsample;
  LsdArgs a{};
  int64_t t[3], c[3], g[3], r[3];
  double sv[3];
  for (int d = 0; d < 3; ++d) {
    if (tile_shape[d] < 1 || tile_shape[d] > (1 << 20) || seg_shape[d] < 1) BSMI_FAIL(BSMI_ERR_INVALID, "tile / seg shape out of range on axis %d", d);
    if (chunk_shape[d] < 1) BSMI_FAIL(BSMI_ERR_INVALID, "chunk extent must be positive");
    if (margin[d] < 0 || margin[d] > 4096 || context[d] < 0 || context[d] > 4096)
      BSMI_FAIL(BSMI_ERR_INVALID, "margin / context out of range on axis %d", d);
    if (!(sigma[d] > 0.f) || !(voxel_size[d] > 0.f)) BSMI_FAIL(BSMI_ERR_INVALID, "sigma and voxel_size must be positive");
    t[d] = tile_shape[d];
    c[d] = std::min<int64_t>(chunk_shape[d], t[d]);
    g[d] = c[d] + 2 * margin[d];
    if (g[d] % df || context[d] % df)
      BSMI_FAIL(BSMI_ERR_INVALID, "axis %d: chunk + 2 margin (%lld) and the context (%lld) must be multiples of the downsample factor %d (as the lsd package requires)",
                d, (long long)g[d], (long long)context[d], df);
    // the label array of every chunk must lie in the seg tile (the caller reads the halo, zeros beyond the dataset)
    const int64_t halo = margin[d] + context[d];
    if (seg_origin[d] > -halo || seg_origin[d] + seg_shape[d] < t[d] + halo)
      BSMI_FAIL(BSMI_ERR_INVALID, "axis %d: the seg tile (origin %lld, extent %lld) does not hold the tile (%lld) grown by margin + context (%lld)", d,
                (long long)seg_origin[d], (long long)seg_shape[d], (long long)t[d], (long long)halo);
    sv[d] = (double)sigma[d] / ((double)voxel_size[d] * df);
    r[d] = (int64_t)(3.0 * sv[d] + 0.5);
  }
  const size_t ngroups = (size_t)(2 * r[2] + 1 + kLsdTapBits - 1) / kLsdTapBits;
  const size_t ntab = 3 * (size_t)((2 * r[0] + 1) + (2 * r[1] + 1)) + ngroups * (3 << kLsdTapBits);
  const size_t lds = ntab * sizeof(double) +
                     ((size_t)(kLsdBZ + 2 * r[0]) * (kLsdBY + 2 * r[1]) * (kLsdBX + 2 * r[2]) + kLsdWinPad) * sizeof(uint32_t);
  if (r[0] > 512 || r[1] > 512 || r[2] > 512 || lds > kLsdLdsBytes)
    BSMI_FAIL(BSMI_ERR_INVALID, "LSD window radius (%lld, %lld, %lld) above the kernel's limit (%zu bytes of LDS, %zu needed)", (long long)r[0],
              (long long)r[1], (long long)r[2], kLsdLdsBytes, lds);
  if (count_z_end < 0 || count_z_end > t[0]) BSMI_FAIL(BSMI_ERR_INVALID, "count_z_end outside the tile");
  const int64_t tvox = t[0] * t[1] * t[2];
  const int64_t pvox = (t[0] + 2 * margin[0]) * (t[1] + 2 * margin[1]) * (t[2] + 2 * margin[2]);
  const int64_t gvox = g[0] * g[1] * g[2];
  if (tvox >= (1ll << 36) || pvox >= (1ll << 36) || gvox >= (1ll << 31) || g[0] * g[1] >= (1ll << 31)) BSMI_FAIL(BSMI_ERR_INVALID, "tile too large");
  a.seg = seg_dev; a.pred = pred_dev; a.mask = mask_dev;
  a.tz = (int)t[0]; a.ty = (int)t[1]; a.tx = (int)t[2];
  a.cz = (int)c[0]; a.cy = (int)c[1]; a.cx = (int)c[2];
  a.ncz = ceil_div(a.tz, a.cz); a.ncy = ceil_div(a.ty, a.cy); a.ncx = ceil_div(a.tx, a.cx);
  const int64_t nch64 = (int64_t)a.ncz * a.ncy * a.ncx;
  if (nch64 > 65535) BSMI_FAIL(BSMI_ERR_INVALID, "more than 65535 chunks in one tile");
  const int nch = (int)nch64;
  a.mz = (int)margin[0]; a.my = (int)margin[1]; a.mx = (int)margin[2];
  a.kz = (int)context[0]; a.ky = (int)context[1]; a.kx = (int)context[2];
  a.gz = (int)g[0]; a.gy = (int)g[1]; a.gx = (int)g[2];
  a.sd = (int)((g[0] + 2 * context[0]) / df); a.sh = (int)((g[1] + 2 * context[1]) / df); a.sw = (int)((g[2] + 2 * context[2]) / df);
  a.df = df;
  a.rz = (int)r[0]; a.ry = (int)r[1]; a.rx = (int)r[2];
  a.gvox = gvox;
  a.svox = (int64_t)a.sd * a.sh * a.sw;
  a.sy = (int)seg_shape[1]; a.sx = (int)seg_shape[2];
  a.seg_base = ((-seg_origin[0]) * seg_shape[1] + (-seg_origin[1])) * seg_shape[2] + (-seg_origin[2]);
  a.py = (int)(t[1] + 2 * margin[1]); a.px = (int)(t[2] + 2 * margin[2]);
  a.pvox = pvox;
  for (int d = 0; d < 3; ++d) {
    a.sigma[d] = sigma[d];
    a.step[d] = voxel_size[d] * df;
  }
  a.floor_ = floor_; a.ceil_ = ceil_;
  a.count_z_end = (int)count_z_end;
  a.emap = error_map_dev; a.emask = error_mask_dev;
  a.hist = (unsigned long long*)hist_dev;
  a.dbg_desc = debug_desc_dev;
  BSMI_HIP(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  // scratch of one group of chunks: sub-grid ids, diff, raw / eroded / opened mask
  const size_t sub_b = (size_t)a.svox * 4, diff_b = (size_t)gvox * 4, mask_b = (size_t)gvox;
  const size_t per_chunk = sub_b + diff_b + 3 * mask_b;
  if (per_chunk > scratch_limit_bytes)
    BSMI_FAIL(BSMI_ERR_INVALID, "one chunk needs %zu bytes of scratch, the limit is %llu", per_chunk, (unsigned long long)scratch_limit_bytes);
  const int group = (int)std::min<uint64_t>(scratch_limit_bytes / per_chunk, (uint64_t)nch);
  int rc = grow(&h->lsd_scratch, &h->lsd_scratch_cap, per_chunk * group, s);
  if (rc) return rc;
  rc = grow((void**)&h->cmax, &h->cmax_cap, (size_t)nch * sizeof(uint32_t), s);
  if (rc) return rc;
  rc = grow((void**)&h->lsd_keys, &h->lsd_keys_cap, (h->cap + 1) * sizeof(uint64_t), s);
  if (rc) return rc;
  if (!h->lsd_inserts) BSMI_HIP(hipMalloc((void**)&h->lsd_inserts, sizeof(uint32_t)));
  // window tables as scipy's gaussian_filter1d builds the weights (sigma in sub-grid cells, truncate = 3.0), in float64;
  // coordinates relative to the cell
  const float key[7] = {sigma[0], sigma[1], sigma[2], voxel_size[0], voxel_size[1], voxel_size[2], (float)df};
  if (!h->lsd_w || std::memcmp(key, h->lsd_w_key, sizeof key) != 0) {
    std::vector<double> tab;
    tab.reserve(ntab);
    for (int d = 0; d < 3; ++d) {
      const int n = (int)(2 * r[d] + 1);
      const double step = (double)(voxel_size[d] * df);
      std::vector<double> w(n);
      double sum = 0;
      for (int k = -(int)r[d]; k <= (int)r[d]; ++k) sum += w[k + r[d]] = exp(-0.5 * (double)k * k / (sv[d] * sv[d]));
      auto moment = [&](int i, int p) {  // tap i of the axis: w, w c, w c^2
        const double cc = (i - (int)r[d]) * step;
        return w[i] / sum * (p == 0 ? 1.0 : p == 1 ? cc : cc * cc);
      };
      if (d < 2) {
        for (int p = 0; p < 3; ++p)
          for (int i = 0; i < n; ++i) tab.push_back(moment(i, p));
      } else {
        for (size_t g = 0; g < ngroups; ++g)
          for (uint32_t bits = 0; bits < (1u << kLsdTapBits); ++bits)
            for (int p = 0; p < 3; ++p) {
              double acc = 0;
              for (int b = 0; b < kLsdTapBits; ++b)
                if ((bits >> b & 1) && (int)(g * kLsdTapBits + b) < n) acc += moment((int)(g * kLsdTapBits + b), p);
              tab.push_back(acc);
            }
      }
    }
    rc = grow((void**)&h->lsd_w, &h->lsd_w_cap, ntab * sizeof(double), s);
    if (rc) return rc;
    BSMI_HIP(hipStreamSynchronize(s));  // the host vector must outlive the copy, and earlier launches may still read the old tables
    BSMI_HIP(hipMemcpy(h->lsd_w, tab.data(), ntab * sizeof(double), hipMemcpyHostToDevice));
    std::memcpy(h->lsd_w_key, key, sizeof key);
  }
  a.w = h->lsd_w;
  {
    static DeviceOnce once;
    rc = once.run([&]() -> int {
      BSMI_HIP(hipFuncSetAttribute((const void*)lsd_desc_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLsdLdsBytes));
      return BSMI_OK;
    });
    if (rc) return rc;
  }
  a.keys = h->lsd_keys;
  a.cap = h->cap;
  a.inserts = h->lsd_inserts;
  a.flags = h->flags;
  a.cmax = h->cmax;
  uint8_t* base = (uint8_t*)h->lsd_scratch;
  a.sub = (uint32_t*)base;
  a.diff = (float*)(base + sub_b * group);
  a.raw = base + (sub_b + diff_b) * group;
  a.e1 = a.raw + mask_b * group;
  a.e2 = a.e1 + mask_b * group;
  BSMI_HIP(hipMemsetAsync(h->cmax, 0, (size_t)nch * sizeof(uint32_t), s));
  BSMI_HIP(hipMemsetAsync(h->lsd_keys, 0xff, (h->cap + 1) * sizeof(uint64_t), s));
  BSMI_HIP(hipMemsetAsync(h->lsd_inserts, 0, sizeof(uint32_t), s));
  const dim3 blk(64, 4);
  const int cells_z = a.gz / df, cells_y = a.gy / df, cells_x = a.gx / df;
  const unsigned desc_blocks = (unsigned)(ceil_div(cells_z, kLsdBZ) * ceil_div(cells_y, kLsdBY) * ceil_div(cells_x, kLsdBX));
  for (int c0 = 0; c0 < nch; c0 += group) {
    const unsigned n = (unsigned)std::min(group, nch - c0);
    a.chunk0 = c0;
    hipLaunchKernelGGL(lsd_sub_kernel, dim3((unsigned)std::min<int64_t>(ceil_div64(a.svox, 256), 4096), n), dim3(256), 0, s, a);
    hipLaunchKernelGGL(lsd_desc_kernel, dim3(desc_blocks, n), dim3(256), lds, s, a);
    const dim3 rows_g((unsigned)ceil_div(a.gz * a.gy, kRowsPerBlock), n);
    hipLaunchKernelGGL(lsd_norm_kernel, rows_g, blk, 0, s, a);
    hipLaunchKernelGGL(lsd_xy_kernel<true>, rows_g, blk, 0, s, a, (const uint8_t*)a.raw, a.e1);
    hipLaunchKernelGGL(lsd_xy_kernel<false>, rows_g, blk, 0, s, a, (const uint8_t*)a.e1, a.e2);
    hipLaunchKernelGGL(lsd_zclose_kernel, dim3((unsigned)ceil_div(a.cz * a.cy, kRowsPerBlock), n), blk, 0, s, a);
    BSMI_HIP(hipGetLastError());
    if (debug_diff_dev)
      BSMI_HIP(hipMemcpyAsync(debug_diff_dev + (size_t)c0 * gvox, a.diff, (size_t)n * gvox * 4, hipMemcpyDeviceToDevice, s));
    if (debug_raw_mask_dev)
      BSMI_HIP(hipMemcpyAsync(debug_raw_mask_dev + (size_t)c0 * gvox, a.raw, (size_t)n * gvox, hipMemcpyDeviceToDevice, s));
  }
  if (debug_max_dev) BSMI_HIP(hipMemcpyAsync(debug_max_dev, h->cmax, (size_t)nch * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
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

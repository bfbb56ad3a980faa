// `bs utils` on the device (reference utils.py, data/mask.py, data/scale_pyramid.py, data/bbox.py).
//
// Raw mask: a binary closing of every z section by the disk dx^2 + dy^2 <= r^2, of the section zero-extended to the plane.
// Sections are bit-packed along x, 64 voxels per uint64_t, and the disk is an OR over dy of the row y + dy dilated along x by
// w(dy) = isqrt(r^2 - dy^2).  Dilation along x composes (by a, then by b = by a + b) and commutes with OR, so the rows are
// taken from the widest (dy = 0) outwards: acc = rows(+-a) | smear(acc, w(a - 1) - w(a)).  That is one smear per distinct
// width (seven for r = 10), each a few shifts of a 128-bit window: the word itself with 32 voxels of its neighbours on
// either side, which the at most r <= 16 voxels of smearing never use up.
// Two launches.  The first packs the u8 section with a wave64 __ballot per word, straight into the coordinates of the
// section grown by r on every side (so the dilation is evaluated where the erosion will look), and dilates; its result,
// the packed grown sections, is the work buffer.  The second erodes as ~dilate(~q), on words re-aligned to the section,
// and unpacks to 0 / 1 bytes.  A workgroup keeps its band of packed rows (tile rows + 2 r) in LDS.  Bits outside the grid
// (rows, words, and the pad bits of a row's last word) are 0 in the band of either pass: "outside" for the dilation, and
// for the erosion never read by a voxel of the section, since the grown grid holds the whole disk around each of them.
// Traffic per voxel: 1 byte read (the band's halo re-reads come from L2), 1 byte written, 1/2 byte of packed words.
//
// Scale pyramid: window means (u8, u16; u32 sum, exact) and sampling / repetition (any itemsize), one output voxel per lane.
// Bounding box: a wave per row, min / max x from the ballot of `voxel != 0`, merged into the caller's box with 64-bit atomics.
#include <hip/hip_runtime.h>

#include "../../include/bsmi.h"
#include "common.h"

namespace bsmi {
namespace {

constexpr int kMaxRadius = 16;
constexpr int kTY = 64, kTW = 8;                      // tile: rows x packed words
constexpr int kBandRows = kTY + 2 * kMaxRadius;       // rows of the band in LDS
constexpr int kBandWords = kTW + 2;                   // a word of margin on either side
constexpr int kThreads = 256;

struct Win {   // 128 voxels: lo = bits 0..63
  uint64_t lo, hi;
};

__device__ __forceinline__ Win shl(Win v, int s) {   // 0 < s < 64
  return Win{v.lo << s, (v.hi << s) | (v.lo >> (64 - s))};
}
__device__ __forceinline__ Win shr(Win v, int s) {   // 0 < s < 64
  return Win{(v.lo >> s) | (v.hi << (64 - s)), v.hi >> s};
}
__device__ __forceinline__ Win operator|(Win a, Win b) { return Win{a.lo | b.lo, a.hi | b.hi}; }

// OR of v shifted by every s in [-d, d], 1 <= d <= 16; the d bits at either end of the result are not to be used
__device__ __forceinline__ Win smear(Win v, int d) {
  const int n = 2 * d + 1;   // shifts 0 .. 2 d upwards by doubling, then back down by d
  int c = 1;
  while (2 * c <= n) {
    v = v | shl(v, c);
    c *= 2;
  }
  if (n > c) v = v | shl(v, n - c);
  return shr(v, d);
}

// the window of word j (0 <= j < kTW) of a band row: dwords 2 j + 1 .. 2 j + 4 of the row (word j + 1 is the word itself)
__device__ __forceinline__ Win window(const uint32_t* row, int j) {
  const uint32_t* p = row + 2 * j + 1;
  return Win{(uint64_t)p[0] | (uint64_t)p[1] << 32, (uint64_t)p[2] | (uint64_t)p[3] << 32};
}

// word j of the row whose band row is `centre` (>= r rows from either end of the band), dilated by the disk of radius r
__device__ __forceinline__ uint64_t disk_dilate_word(const uint64_t* band, int centre, int j, int r) {
  const uint32_t* b = (const uint32_t*)band;
  constexpr int stride = 2 * kBandWords;
  Win acc = window(b + centre * stride, j);
  int w = r;   // isqrt(r^2 - a^2) at a = 0
  for (int a = 1; a <= r; ++a) {
    int wa = w;
    while (wa * wa + a * a > r * r) --wa;
    if (wa < w) acc = smear(acc, w - wa);
    w = wa;
    acc = acc | window(b + (centre - a) * stride, j) | window(b + (centre + a) * stride, j);
  }
  // w(r) = 0: nothing left to smear
  return (acc.lo >> 32) | (acc.hi << 32);
}

// grid: (tiles of the grown grid along x, along y, sections).  q [D][H + 2 r][wg] packed, grown coordinates (gy, gx) = (y + r, x + r)
__global__ void __launch_bounds__(kThreads) closing_dilate_kernel(const uint8_t* __restrict__ in, uint64_t* __restrict__ q, int H, int W, int r, int wg) {
  __shared__ uint64_t band[kBandRows * kBandWords];
  const int z = blockIdx.z, hg = H + 2 * r;
  const int gy0 = blockIdx.y * kTY, m0 = blockIdx.x * kTW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rows = kTY + 2 * r;
  const uint8_t* sec = in + (int64_t)z * H * W;
  // band row b = grown row gy0 - r + b = section row gy0 - 2 r + b; band word k = grown word m0 - 1 + k
  for (int i = wave; i < rows * kBandWords; i += kThreads / 64) {
    const int b = i / kBandWords, k = i - b * kBandWords;
    const int y = gy0 - 2 * r + b;
    const int64_t x0 = (int64_t)(m0 - 1 + k) * 64 - r;   // section x of the word's bit 0
    uint64_t bits = 0;
    if (y >= 0 && y < H && x0 + 63 >= 0 && x0 < W) {   // uniform in the wave
      const int64_t x = x0 + lane;
      const bool set = x >= 0 && x < W && sec[(int64_t)y * W + x] != 0;
      bits = __ballot(set);
    }
    if (lane == 0) band[i] = bits;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < kTY * kTW; t += kThreads) {
    const int ty = t / kTW, j = t - ty * kTW;
    const int gy = gy0 + ty, m = m0 + j;
    if (gy >= hg || m >= wg) continue;
    q[((int64_t)z * hg + gy) * wg + m] = disk_dilate_word(band, ty + r, j, r);
  }
}

// grid: (tiles of the section along x, along y, sections).  WIDE: four voxels per store (W a multiple of 4, out 4-byte aligned)
template <bool WIDE>
__global__ void __launch_bounds__(kThreads) closing_erode_kernel(const uint64_t* __restrict__ q, uint8_t* __restrict__ out, int H, int W, int r, int wg) {
  __shared__ uint64_t band[kBandRows * kBandWords];
  __shared__ uint64_t res[kTY * kTW];
  const int z = blockIdx.z, hg = H + 2 * r;
  const int y0 = blockIdx.y * kTY, j0 = blockIdx.x * kTW;
  const int rows = kTY + 2 * r;
  const int64_t valid = (int64_t)W + 2 * r;   // bits of a grown row
  const uint64_t* sec = q + (int64_t)z * hg * wg;
  // ~q with everything outside the grown grid 0, as word m of the grown row
  auto inverted = [&](int gy, int m) -> uint64_t {
    if (m < 0 || m >= wg) return 0;
    const int64_t left = valid - ((int64_t)m << 6);   // valid bits from this word on (>= 1)
    const uint64_t mask = left >= 64 ? ~0ull : (1ull << left) - 1;
    return ~sec[(int64_t)gy * wg + m] & mask;
  };
  // band row b = grown row y0 + b (the rows y - r .. y + r of section row y are the grown rows y .. y + 2 r); band word k = section
  // word j0 - 1 + k, whose bit 0 is grown bit 64 (j0 - 1 + k) + r
  for (int i = threadIdx.x; i < rows * kBandWords; i += kThreads) {
    const int b = i / kBandWords, k = i - b * kBandWords;
    const int gy = y0 + b, m = j0 - 1 + k;
    uint64_t bits = 0;
    if (gy < hg) bits = (inverted(gy, m) >> r) | (inverted(gy, m + 1) << (64 - r));
    band[i] = bits;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < kTY * kTW; t += kThreads) {
    const int ty = t / kTW, j = t - ty * kTW;
    if (y0 + ty >= H || ((int64_t)(j0 + j) << 6) >= W) continue;   // never unpacked
    res[t] = ~disk_dilate_word(band, ty + r, j, r);
  }
  __syncthreads();
  uint8_t* osec = out + (int64_t)z * H * W;
  if (WIDE) {
    for (int t = threadIdx.x; t < kTY * kTW * 16; t += kThreads) {
      const int ty = t / (kTW * 16), g = t - ty * (kTW * 16);   // g: group of four voxels in the tile row
      const int y = y0 + ty;
      const int64_t x = ((int64_t)j0 << 6) + 4 * g;
      if (y >= H || x >= W) continue;
      const uint32_t nib = (uint32_t)(res[ty * kTW + (g >> 4)] >> (4 * (g & 15))) & 15u;
      *(uint32_t*)(osec + (int64_t)y * W + x) = (nib & 1u) | (nib & 2u) << 7 | (nib & 4u) << 14 | (nib & 8u) << 21;
    }
  } else {
    for (int t = threadIdx.x; t < kTY * kTW * 64; t += kThreads) {
      const int ty = t / (kTW * 64), g = t - ty * (kTW * 64);
      const int y = y0 + ty;
      const int64_t x = ((int64_t)j0 << 6) + g;
      if (y >= H || x >= W) continue;
      osec[(int64_t)y * W + x] = (uint8_t)(res[ty * kTW + (g >> 6)] >> (g & 63) & 1);
    }
  }
}

struct Scale {
  int64_t in[3], out[3];
  int k[3], lead[3];
};

template <typename T>
__global__ void __launch_bounds__(256) downscale_mean_kernel(const T* __restrict__ in, T* __restrict__ out, Scale s, uint32_t window) {
  const int64_t n = s.out[0] * s.out[1] * s.out[2];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t ox = i % s.out[2], oy = i / s.out[2] % s.out[1], oz = i / (s.out[2] * s.out[1]);
    const int64_t z0 = oz * s.k[0] - s.lead[0], y0 = oy * s.k[1] - s.lead[1], x0 = ox * s.k[2] - s.lead[2];
    uint32_t sum = 0;
    for (int dz = 0; dz < s.k[0]; ++dz) {
      const int64_t z = z0 + dz;
      if (z < 0 || z >= s.in[0]) continue;
      for (int dy = 0; dy < s.k[1]; ++dy) {
        const int64_t y = y0 + dy;
        if (y < 0 || y >= s.in[1]) continue;
        const T* row = in + (z * s.in[1] + y) * s.in[2];
        for (int dx = 0; dx < s.k[2]; ++dx) {
          const int64_t x = x0 + dx;
          if (x >= 0 && x < s.in[2]) sum += row[x];
        }
      }
    }
    out[i] = (T)(sum / window);
  }
}

template <typename T, bool UP>
__global__ void __launch_bounds__(256) rescale_sample_kernel(const T* __restrict__ in, T* __restrict__ out, Scale s) {
  const int64_t n = s.out[0] * s.out[1] * s.out[2];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t o[3] = {i / (s.out[2] * s.out[1]), i / s.out[2] % s.out[1], i % s.out[2]};
    int64_t at = 0;
    bool inside = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int64_t p = UP ? o[d] / s.k[d] : o[d] * s.k[d] + s.k[d] / 2 - s.lead[d];
      inside = inside && p >= 0 && p < s.in[d];
      at = at * s.in[d] + p;
    }
    out[i] = inside ? in[at] : (T)0;
  }
}

// a wave per row (z, y) of the tile; box = (min z, y, x, max z, y, x) of the non-zero voxels, origin added
template <typename T>
__global__ void __launch_bounds__(256) nonzero_bbox_kernel(const T* __restrict__ in, int64_t D, int64_t H, int64_t W, int64_t oz, int64_t oy, int64_t ox,
                                                           long long* __restrict__ box) {
  const int lane = threadIdx.x & 63;
  const int64_t nrows = D * H;
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x / 64);
  const long long big = 0x7fffffffffffffffll;
  long long lo[3] = {big, big, big}, hi[3] = {-1, -1, -1};
  for (int64_t row = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); row < nrows; row += nwaves) {
    long long x_lo = big, x_hi = -1;
    for (int64_t x0 = 0; x0 < W; x0 += 64) {
      const int64_t x = x0 + lane;
      const uint64_t m = __ballot(x < W && in[row * W + x] != 0);
      if (m) {
        x_lo = min(x_lo, (long long)(x0 + __ffsll((unsigned long long)m) - 1));
        x_hi = max(x_hi, (long long)(x0 + 63 - __clzll((long long)m)));
      }
    }
    if (x_hi >= 0) {
      const long long z = row / H, y = row - z * H;
      lo[0] = min(lo[0], z), lo[1] = min(lo[1], y), lo[2] = min(lo[2], x_lo);
      hi[0] = max(hi[0], z), hi[1] = max(hi[1], y), hi[2] = max(hi[2], x_hi);
    }
  }
  if (lane == 0 && hi[0] >= 0) {
    const long long org[3] = {oz, oy, ox};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      atomicMin(&box[d], lo[d] + org[d]);
      atomicMax(&box[3 + d], hi[d] + org[d]);
    }
  }
}

bool bad_shape(const int64_t shape[3]) {
  for (int d = 0; d < 3; ++d)
    if (shape[d] < 0 || shape[d] > (1 << 20)) return true;
  return false;
}

int scale_args(const int64_t in_shape[3], const int32_t factor[3], const int32_t lead[3], const int64_t out_shape[3], Scale* s, int64_t* window) {
  if (!in_shape || !factor || !lead || !out_shape) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (bad_shape(in_shape) || bad_shape(out_shape)) BSMI_FAIL(BSMI_ERR_INVALID, "shape out of range");
  *window = 1;
  for (int d = 0; d < 3; ++d) {
    if (factor[d] < 1 || factor[d] > 65536) BSMI_FAIL(BSMI_ERR_INVALID, "factor %d on axis %d: 1..65536", factor[d], d);
    if (lead[d] < 0 || lead[d] >= factor[d]) BSMI_FAIL(BSMI_ERR_INVALID, "lead %d on axis %d: 0 <= lead < factor", lead[d], d);
    s->in[d] = in_shape[d];
    s->out[d] = out_shape[d];
    s->k[d] = factor[d];
    s->lead[d] = lead[d];
    *window *= factor[d];
  }
  return BSMI_OK;
}

unsigned grid_for(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 65536); }

}  // namespace
}  // namespace bsmi

using namespace bsmi;

extern "C" {

size_t bsmi_mask_closing_work_bytes(const int64_t shape[3], int radius) {
  if (!shape || radius < 1 || radius > kMaxRadius || bad_shape(shape)) return 0;
  const size_t hg = (size_t)shape[1] + 2 * radius, wg = ((size_t)shape[2] + 2 * radius + 63) / 64;
  return (size_t)shape[0] * hg * wg * sizeof(uint64_t);
}

int bsmi_mask_closing_disk_u8(int device, const uint8_t* in_dev, const int64_t shape[3], int radius, uint8_t* out_dev, void* work_dev,
                              size_t work_bytes, void* stream) {
  if (!in_dev || !shape || !out_dev || !work_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (radius < 1 || radius > kMaxRadius) BSMI_FAIL(BSMI_ERR_INVALID, "radius %d: 1..%d", radius, kMaxRadius);
  if (bad_shape(shape)) BSMI_FAIL(BSMI_ERR_INVALID, "shape out of range");
  if (in_dev == out_dev || work_dev == (const void*)in_dev || work_dev == (void*)out_dev)
    BSMI_FAIL(BSMI_ERR_INVALID, "in, out and work must be different buffers");
  if ((uintptr_t)work_dev % 8) BSMI_FAIL(BSMI_ERR_INVALID, "work_dev must be 8-byte aligned");
  const size_t need = bsmi_mask_closing_work_bytes(shape, radius);
  if (work_bytes < need) BSMI_FAIL(BSMI_ERR_INVALID, "work buffer of %zu bytes: bsmi_mask_closing_work_bytes asks for %zu", work_bytes, need);
  const int D = (int)shape[0], H = (int)shape[1], W = (int)shape[2];
  if (D == 0 || H == 0 || W == 0) return BSMI_OK;
  if (D > 65535) BSMI_FAIL(BSMI_ERR_INVALID, "%d sections: at most 65535 in one call", D);
  const int hg = H + 2 * radius, wg = (W + 2 * radius + 63) / 64;
  BSMI_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(kThreads);
  const dim3 grid1(ceil_div(wg, kTW), ceil_div(hg, kTY), D), grid2(ceil_div(ceil_div(W, 64), kTW), ceil_div(H, kTY), D);
  if (grid1.y > 65535) BSMI_FAIL(BSMI_ERR_INVALID, "%d rows: too many for one call", H);
  hipLaunchKernelGGL(closing_dilate_kernel, grid1, blk, 0, s, in_dev, (uint64_t*)work_dev, H, W, radius, wg);
  if (W % 4 == 0 && (uintptr_t)out_dev % 4 == 0)
    hipLaunchKernelGGL(closing_erode_kernel<true>, grid2, blk, 0, s, (const uint64_t*)work_dev, out_dev, H, W, radius, wg);
  else
    hipLaunchKernelGGL(closing_erode_kernel<false>, grid2, blk, 0, s, (const uint64_t*)work_dev, out_dev, H, W, radius, wg);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_downscale_mean(int device, const void* in_dev, int itemsize, const int64_t in_shape[3], const int32_t factor[3], const int32_t lead[3],
                        void* out_dev, const int64_t out_shape[3], void* stream) {
  if (!in_dev || !out_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (in_dev == out_dev) BSMI_FAIL(BSMI_ERR_INVALID, "in and out must be different buffers");
  if (itemsize != 1 && itemsize != 2) BSMI_FAIL(BSMI_ERR_INVALID, "itemsize %d: 1 (u8) or 2 (u16)", itemsize);
  Scale sc;
  int64_t window;
  const int rc = scale_args(in_shape, factor, lead, out_shape, &sc, &window);
  if (rc != BSMI_OK) return rc;
  if (window > 65536) BSMI_FAIL(BSMI_ERR_INVALID, "window of %lld voxels: at most 65536 (u32 sum)", (long long)window);
  const int64_t n = sc.out[0] * sc.out[1] * sc.out[2];
  if (n == 0) return BSMI_OK;
  BSMI_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  if (itemsize == 1)
    hipLaunchKernelGGL(downscale_mean_kernel<uint8_t>, dim3(grid_for(n)), dim3(256), 0, s, (const uint8_t*)in_dev, (uint8_t*)out_dev, sc, (uint32_t)window);
  else
    hipLaunchKernelGGL(downscale_mean_kernel<uint16_t>, dim3(grid_for(n)), dim3(256), 0, s, (const uint16_t*)in_dev, (uint16_t*)out_dev, sc, (uint32_t)window);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

#define BSMI_SAMPLE(T)                                                                                                                 \
  do {                                                                                                                                 \
    if (mode == BSMI_RESCALE_UP)                                                                                                       \
      hipLaunchKernelGGL((rescale_sample_kernel<T, true>), dim3(grid_for(n)), dim3(256), 0, s, (const T*)in_dev, (T*)out_dev, sc);     \
    else                                                                                                                               \
      hipLaunchKernelGGL((rescale_sample_kernel<T, false>), dim3(grid_for(n)), dim3(256), 0, s, (const T*)in_dev, (T*)out_dev, sc);    \
  } while (0)

int bsmi_rescale_sample(int device, const void* in_dev, int itemsize, const int64_t in_shape[3], const int32_t factor[3], const int32_t lead[3],
                        int mode, void* out_dev, const int64_t out_shape[3], void* stream) {
  if (!in_dev || !out_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (in_dev == out_dev) BSMI_FAIL(BSMI_ERR_INVALID, "in and out must be different buffers");
  if (itemsize != 1 && itemsize != 2 && itemsize != 4 && itemsize != 8) BSMI_FAIL(BSMI_ERR_INVALID, "itemsize %d: 1, 2, 4 or 8", itemsize);
  if (mode != BSMI_RESCALE_DOWN && mode != BSMI_RESCALE_UP) BSMI_FAIL(BSMI_ERR_INVALID, "mode %d: BSMI_RESCALE_DOWN or BSMI_RESCALE_UP", mode);
  Scale sc;
  int64_t window;
  const int rc = scale_args(in_shape, factor, lead, out_shape, &sc, &window);
  if (rc != BSMI_OK) return rc;
  if (mode == BSMI_RESCALE_UP)
    for (int d = 0; d < 3; ++d)
      if (lead[d] != 0 || out_shape[d] > in_shape[d] * factor[d])
        BSMI_FAIL(BSMI_ERR_INVALID, "up: lead must be 0 and out_shape at most in_shape * factor (axis %d)", d);
  const int64_t n = sc.out[0] * sc.out[1] * sc.out[2];
  if (n == 0) return BSMI_OK;
  BSMI_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  if (itemsize == 1) BSMI_SAMPLE(uint8_t);
  else if (itemsize == 2) BSMI_SAMPLE(uint16_t);
  else if (itemsize == 4) BSMI_SAMPLE(uint32_t);
  else BSMI_SAMPLE(uint64_t);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}
#undef BSMI_SAMPLE

int bsmi_nonzero_bbox(int device, const void* in_dev, int itemsize, const int64_t shape[3], const int64_t origin[3], int64_t* box_dev, void* stream) {
  if (!in_dev || !shape || !origin || !box_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (itemsize != 1 && itemsize != 2 && itemsize != 4 && itemsize != 8) BSMI_FAIL(BSMI_ERR_INVALID, "itemsize %d: 1, 2, 4 or 8", itemsize);
  if (bad_shape(shape)) BSMI_FAIL(BSMI_ERR_INVALID, "shape out of range");
  for (int d = 0; d < 3; ++d)
    if (origin[d] < 0 || origin[d] > (1ll << 40)) BSMI_FAIL(BSMI_ERR_INVALID, "origin out of range on axis %d", d);
  const int64_t rows = shape[0] * shape[1];
  if (rows == 0 || shape[2] == 0) return BSMI_OK;
  BSMI_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)std::min<int64_t>((rows + 3) / 4, 4096)), blk(256);
  long long* box = (long long*)box_dev;
#define BSMI_BBOX(T) \
  hipLaunchKernelGGL(nonzero_bbox_kernel<T>, grid, blk, 0, s, (const T*)in_dev, shape[0], shape[1], shape[2], origin[0], origin[1], origin[2], box)
  if (itemsize == 1) BSMI_BBOX(uint8_t);
  else if (itemsize == 2) BSMI_BBOX(uint16_t);
  else if (itemsize == 4) BSMI_BBOX(uint32_t);
  else BSMI_BBOX(uint64_t);
#undef BSMI_BBOX
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

}  // extern "C"

// Intensity training augmentation of raw (include/bsmi.h, "training augmentation: the intensity chain"; the rules in full:
// DESIGN.md section 7k, tests/intensity_ref.py): NoiseAugment, IntensityAugment, GammaAugment, ImpulseNoiseAugment,
// SmoothAugment and DefectAugment on a float32 block in [0, 1], one launch per node.  Section statistics fall between the
// nodes, so the chain cannot be one epilogue of the resampling: bsmi_aug_section_stats reduces every section in a fixed
// order (per-workgroup partials, combined in index order; no float atomics), so one plan gives one result, bit for bit.
// All of it is memory-bound and small (1.2 M voxels at the 3d_mtlsd shape): lanes run along x, rows are read and written
// whole.  Every random scalar is drawn by the caller; the per-voxel ones come from Philox4x32-10 keyed by the caller's seed.
#include "common.h"
#include "augment_intensity.h"

namespace bsmi {
namespace {

using namespace augi;

struct Block {
  uint32_t total;   // D * H * W, fewer than 2^31
  uint32_t plane;   // H * W
};

// x = clip(x + sigma * n), n = sqrt(-2 ln u1) cos(2 pi u2) from words 0 and 1 of the voxel's Philox output
__global__ __launch_bounds__(256) void aug_noise_kernel(Block g, float* __restrict__ x, uint32_t k0, uint32_t k1, float sigma) {
  for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < g.total; idx += gridDim.x * blockDim.x) {
    x[idx] = noise_value(x[idx], idx, k0, k1, sigma);
  }
}

// a voxel is replaced iff word 2 < threshold (threshold 2^32: always), by (word 3 >> 8) * 2^-24
__global__ __launch_bounds__(256) void aug_impulse_kernel(Block g, float* __restrict__ x, uint32_t k0, uint32_t k1, uint64_t threshold) {
  for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < g.total; idx += gridDim.x * blockDim.x) {
    float v;
    if (impulse_value(idx, k0, k1, threshold, &v)) x[idx] = v;
  }
}

// Partial (sum, min, max) of chunk blockIdx.x of section blockIdx.y.  The order is fixed by the shape alone: thread t adds
// the chunk's elements t, t + 256, ... in that order, then a binary tree over the 256 threads in LDS.
__global__ __launch_bounds__(256) void aug_stats_partial_kernel(Block g, const float* __restrict__ x, float* __restrict__ partials) {
  __shared__ float ssum[256], smin[256], smax[256];
  const uint32_t chunk = (g.plane + kStatParts - 1) / kStatParts;
  const uint32_t lo = min(blockIdx.x * chunk, g.plane), hi = min(lo + chunk, g.plane);
  const float* sec = x + (size_t)blockIdx.y * g.plane;
  float s = 0.0f, mn = INFINITY, mx = -INFINITY;
  for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) {
    const float v = sec[i];
    s += v;
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  ssum[threadIdx.x] = s, smin[threadIdx.x] = mn, smax[threadIdx.x] = mx;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      ssum[threadIdx.x] += ssum[threadIdx.x + w];
      smin[threadIdx.x] = fminf(smin[threadIdx.x], smin[threadIdx.x + w]);
      smax[threadIdx.x] = fmaxf(smax[threadIdx.x], smax[threadIdx.x + w]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float* p = partials + ((size_t)blockIdx.y * kStatParts + blockIdx.x) * 3;
    p[0] = ssum[0], p[1] = smin[0], p[2] = smax[0];
  }
}

// the partials of a section combined in index order: stats [D][3] = (mean, min, max)
__global__ __launch_bounds__(64) void aug_stats_combine_kernel(int D, float count, const float* __restrict__ partials, float* __restrict__ stats) {
  const int z = blockIdx.x * blockDim.x + threadIdx.x;
  if (z >= D) return;
  const float* p = partials + (size_t)z * kStatParts * 3;
  float s = 0.0f, mn = INFINITY, mx = -INFINITY;
  for (int i = 0; i < kStatParts; ++i) {
    s += p[3 * i];
    mn = fminf(mn, p[3 * i + 1]);
    mx = fmaxf(mx, p[3 * i + 2]);
  }
  stats[3 * z] = s / count, stats[3 * z + 1] = mn, stats[3 * z + 2] = mx;
}

// x = clip(m_z + (x - m_z) * scale_z + shift_z)
__global__ __launch_bounds__(256) void aug_intensity_kernel(Block g, float* __restrict__ x, const float* __restrict__ stats,
                                                            const float* __restrict__ scale, const float* __restrict__ shift) {
  for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < g.total; idx += gridDim.x * blockDim.x) {
    const uint32_t z = idx / g.plane;
    x[idx] = intensity_value(x[idx], stats[3 * z], scale[z], shift[z]);
  }
}

// x = ((x - a) / (b - a))^g (b - a) + a where b - a > 1e-3, a and b the section's extrema; the base 0 (x = a) gives a, and
// the result is held to [a, b], which the exact expression never leaves
__global__ __launch_bounds__(256) void aug_gamma_kernel(Block g, float* __restrict__ x, const float* __restrict__ stats,
                                                        const float* __restrict__ gamma) {
  for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < g.total; idx += gridDim.x * blockDim.x) {
    const uint32_t z = idx / g.plane;
    const float a = stats[3 * z + 1], b = stats[3 * z + 2];
    const float range = b - a;
    if (!(range > 1e-3f)) continue;
    x[idx] = gamma_value(x[idx], a, b, range, gamma[z]);
  }
}

// mode_z: 0 unchanged, 1 / 2 the section becomes 0 / 1, 3 x = m_z + (x - m_z) * contrast_scale; then 2 x - 1 if final_map
__global__ __launch_bounds__(256) void aug_defect_kernel(Block g, float* __restrict__ x, const float* __restrict__ stats,
                                                         const int32_t* __restrict__ mode, float contrast_scale, int final_map) {
  for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < g.total; idx += gridDim.x * blockDim.x) {
    const uint32_t z = idx / g.plane;
    x[idx] = defect_value(x[idx], mode ? mode[z] : 0, stats + 3 * z, contrast_scale, final_map);
  }
}

struct Taps {
  int radius;
  float w[2 * kMaxRadius + 1];
};

// the z pass: whole rows, one tap per section read
__global__ __launch_bounds__(256) void aug_smooth_z_kernel(Block g, int D, Taps t, const float* __restrict__ in, float* __restrict__ out) {
  for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < g.total; idx += gridDim.x * blockDim.x) {
    const int z = (int)(idx / g.plane);
    const uint32_t p = idx - (uint32_t)z * g.plane;
    out[idx] = tap_sum(t.radius, t.w, [&](int k) { return in[(size_t)reflect(z + k - t.radius, D) * g.plane + p]; });
  }
}

// the y and x passes from one tile staged with its halo in LDS: y into `mid` (halo columns included), x out of it
__global__ __launch_bounds__(256) void aug_smooth_yx_kernel(int H, int W, Taps t, const float* __restrict__ in, float* __restrict__ out) {
  const size_t sec = (size_t)blockIdx.z * H * W;
  smooth_yx_tile(H, W, t.radius, t.w, in + sec, out + sec);
}

unsigned grid_of(size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, 2048); }

int block_of(const int64_t shape[3], Block* g) {
  if (!shape) BSMI_FAIL(BSMI_ERR_INVALID, "null shape");
  for (int d = 0; d < 3; ++d)
    if (shape[d] < 1 || shape[d] > (1 << 20)) BSMI_FAIL(BSMI_ERR_INVALID, "block: shape out of range on axis %d", d);
  const unsigned __int128 v = (unsigned __int128)shape[0] * shape[1] * shape[2];
  if (v >= (1ull << 31)) BSMI_FAIL(BSMI_ERR_INVALID, "block: 2^31 voxels or more");
  if (shape[0] > 65535) BSMI_FAIL(BSMI_ERR_INVALID, "block: more than 65535 sections");
  *g = Block{(uint32_t)v, (uint32_t)(shape[1] * shape[2])};
  return BSMI_OK;
}

}  // namespace
}  // namespace bsmi

using namespace bsmi;

extern "C" {

int bsmi_aug_noise_f32(int device, const int64_t shape[3], float* x_dev, uint64_t seed, float sigma, void* stream) {
  Block g;
  if (int rc = block_of(shape, &g)) return rc;
  if (!x_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (!(sigma >= 0.0f) || !(sigma < 1e6f)) BSMI_FAIL(BSMI_ERR_INVALID, "noise sigma must be finite and not negative");
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(aug_noise_kernel, dim3(grid_of(g.total)), dim3(256), 0, (hipStream_t)stream, g, x_dev, (uint32_t)seed, (uint32_t)(seed >> 32),
                     sigma);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_aug_impulse_f32(int device, const int64_t shape[3], float* x_dev, uint64_t seed, uint64_t threshold, void* stream) {
  Block g;
  if (int rc = block_of(shape, &g)) return rc;
  if (!x_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (threshold > (1ull << 32)) BSMI_FAIL(BSMI_ERR_INVALID, "impulse threshold above 2^32");
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(aug_impulse_kernel, dim3(grid_of(g.total)), dim3(256), 0, (hipStream_t)stream, g, x_dev, (uint32_t)seed,
                     (uint32_t)(seed >> 32), threshold);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_aug_section_stats_f32(int device, const int64_t shape[3], const float* x_dev, float* partials_dev, float* stats_dev, void* stream) {
  Block g;
  if (int rc = block_of(shape, &g)) return rc;
  if (!x_dev || !partials_dev || !stats_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  const int D = (int)shape[0];
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(aug_stats_partial_kernel, dim3(kStatParts, D), dim3(256), 0, (hipStream_t)stream, g, x_dev, partials_dev);
  BSMI_HIP(hipGetLastError());
  hipLaunchKernelGGL(aug_stats_combine_kernel, dim3((D + 63) / 64), dim3(64), 0, (hipStream_t)stream, D, (float)g.plane, partials_dev, stats_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_aug_intensity_f32(int device, const int64_t shape[3], float* x_dev, const float* stats_dev, const float* scale_dev, const float* shift_dev,
                           void* stream) {
  Block g;
  if (int rc = block_of(shape, &g)) return rc;
  if (!x_dev || !stats_dev || !scale_dev || !shift_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(aug_intensity_kernel, dim3(grid_of(g.total)), dim3(256), 0, (hipStream_t)stream, g, x_dev, stats_dev, scale_dev, shift_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_aug_gamma_f32(int device, const int64_t shape[3], float* x_dev, const float* stats_dev, const float* gamma_dev, void* stream) {
  Block g;
  if (int rc = block_of(shape, &g)) return rc;
  if (!x_dev || !stats_dev || !gamma_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(aug_gamma_kernel, dim3(grid_of(g.total)), dim3(256), 0, (hipStream_t)stream, g, x_dev, stats_dev, gamma_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_aug_smooth_f32(int device, const int64_t shape[3], float* x_dev, float* tmp_dev, const float* weights, int radius, void* stream) {
  Block g;
  if (int rc = block_of(shape, &g)) return rc;
  if (!x_dev || !tmp_dev || !weights) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (radius < 0 || radius > kMaxRadius) BSMI_FAIL(BSMI_ERR_INVALID, "smoothing radius %d: 0 .. %d", radius, kMaxRadius);
  Taps t{};
  t.radius = radius;
  for (int k = 0; k <= 2 * radius; ++k) t.w[k] = weights[k];
  const int D = (int)shape[0], H = (int)shape[1], W = (int)shape[2];
  const unsigned gy = (unsigned)((H + kTileY - 1) / kTileY);
  if (gy > 65535) BSMI_FAIL(BSMI_ERR_INVALID, "block: more than %d rows", 65535 * kTileY);
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(aug_smooth_z_kernel, dim3(grid_of(g.total)), dim3(256), 0, (hipStream_t)stream, g, D, t, x_dev, tmp_dev);
  BSMI_HIP(hipGetLastError());
  hipLaunchKernelGGL(aug_smooth_yx_kernel, dim3((unsigned)((W + kTileX - 1) / kTileX), gy, (unsigned)D), dim3(256), 0, (hipStream_t)stream, H, W, t,
                     tmp_dev, x_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_aug_defect_f32(int device, const int64_t shape[3], float* x_dev, const float* stats_dev, const int32_t* mode_dev, float contrast_scale,
                        int final_map, void* stream) {
  Block g;
  if (int rc = block_of(shape, &g)) return rc;
  if (!x_dev || (mode_dev && !stats_dev)) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(aug_defect_kernel, dim3(grid_of(g.total)), dim3(256), 0, (hipStream_t)stream, g, x_dev, stats_dev, mode_dev, contrast_scale,
                     final_map ? 1 : 0);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

}  // extern "C"

// Intensity training augmentation of the 2-D setups, a whole batch per launch (include/bsmi.h, "training augmentation of the
// 2-D setups: the intensity chain"; the rules in full: DESIGN.md sections 7k and 7m, tests/aug2d_intensity_ref.py).  A step of a
// 2-D setup is S independent draws of K adjacent sections each (gp.Stack(10)), every draw with its own coins, seed, sigma and
// per-section numbers, held in the trainer's layout [K][S][H][W]: the sections of a draw are S planes apart.  Each node is ONE
// launch for all draws, indexed by a table of per-draw descriptors (bsmi_aug2d_idraw) and per-plane tables (plane p = k S + s);
// a draw without the node leaves its planes alone.  The per-voxel arithmetic is that of the per-block chain, the same device
// code (augment_intensity.h), so draw s comes out as the block (K, H, W) of its sections does from augment_intensity.hip, bit
// for bit.  Small and memory-bound (1.15 M voxels at the 2d_mtlsd shape): grid.y runs over the planes, lanes along x.
#include "common.h"
#include "augment_intensity.h"

namespace bsmi {
namespace {

using namespace augi;

struct Batch {
  int S, K, H, W;
  uint32_t plane;   // H * W; K * S * plane < 2^31
};

// plane blockIdx.y = k * S + s: its section k, its draw's descriptor
__device__ __forceinline__ bsmi_aug2d_idraw draw_of(const Batch& g, const bsmi_aug2d_idraw* __restrict__ idraws, int* k) {
  const int p = (int)blockIdx.y;
  *k = p / g.S;
  return idraws[p - *k * g.S];
}

// the Philox counter is the voxel's linear index inside the draw's own stack: k * H * W + i
__global__ __launch_bounds__(256) void aug2d_noise_kernel(Batch g, const bsmi_aug2d_idraw* __restrict__ idraws, float* __restrict__ xb) {
  int k;
  const bsmi_aug2d_idraw d = draw_of(g, idraws, &k);
  if (!(d.nodes & BSMI_AUG2D_NOISE)) return;
  float* __restrict__ x = xb + (size_t)blockIdx.y * g.plane;
  const uint32_t base = (uint32_t)k * g.plane, k0 = (uint32_t)d.seed, k1 = (uint32_t)(d.seed >> 32);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < g.plane; i += gridDim.x * blockDim.x)
    x[i] = noise_value(x[i], base + i, k0, k1, d.noise_sigma);
}

__global__ __launch_bounds__(256) void aug2d_impulse_kernel(Batch g, const bsmi_aug2d_idraw* __restrict__ idraws, float* __restrict__ xb) {
  int k;
  const bsmi_aug2d_idraw d = draw_of(g, idraws, &k);
  if (!(d.nodes & BSMI_AUG2D_IMPULSE)) return;
  float* __restrict__ x = xb + (size_t)blockIdx.y * g.plane;
  const uint32_t base = (uint32_t)k * g.plane, k0 = (uint32_t)d.seed, k1 = (uint32_t)(d.seed >> 32);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < g.plane; i += gridDim.x * blockDim.x) {
    float v;
    if (impulse_value(base + i, k0, k1, d.impulse_threshold, &v)) x[i] = v;
  }
}

__global__ __launch_bounds__(256) void aug2d_intensity_kernel(Batch g, const bsmi_aug2d_idraw* __restrict__ idraws, float* __restrict__ xb,
                                                              const float* __restrict__ stats, const float* __restrict__ scale,
                                                              const float* __restrict__ shift) {
  int k;
  const bsmi_aug2d_idraw d = draw_of(g, idraws, &k);
  if (!(d.nodes & BSMI_AUG2D_INTENSITY)) return;
  const int p = (int)blockIdx.y;
  float* __restrict__ x = xb + (size_t)p * g.plane;
  const float m = stats[3 * p], sc = scale[p], sh = shift[p];
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < g.plane; i += gridDim.x * blockDim.x) x[i] = intensity_value(x[i], m, sc, sh);
}

__global__ __launch_bounds__(256) void aug2d_gamma_kernel(Batch g, const bsmi_aug2d_idraw* __restrict__ idraws, float* __restrict__ xb,
                                                          const float* __restrict__ stats, const float* __restrict__ gamma) {
  int k;
  const bsmi_aug2d_idraw d = draw_of(g, idraws, &k);
  if (!(d.nodes & BSMI_AUG2D_GAMMA)) return;
  const int p = (int)blockIdx.y;
  float* __restrict__ x = xb + (size_t)p * g.plane;
  const float a = stats[3 * p + 1], b = stats[3 * p + 2], ex = gamma[p];
  const float range = b - a;
  if (!(range > 1e-3f)) return;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < g.plane; i += gridDim.x * blockDim.x) x[i] = gamma_value(x[i], a, b, range, ex);
}

// the defect of draws with the node (mode per plane), then 2 x - 1 of every touched draw if final_map
__global__ __launch_bounds__(256) void aug2d_defect_kernel(Batch g, const bsmi_aug2d_idraw* __restrict__ idraws, float* __restrict__ xb,
                                                           const float* __restrict__ stats, const int32_t* __restrict__ mode, int final_map) {
  int k;
  const bsmi_aug2d_idraw d = draw_of(g, idraws, &k);
  const int p = (int)blockIdx.y;
  const int md = (d.nodes & BSMI_AUG2D_DEFECT) ? mode[p] : 0;
  const int fin = final_map && (d.nodes & BSMI_AUG2D_TOUCHED);
  if (!md && !fin) return;
  float* __restrict__ x = xb + (size_t)p * g.plane;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < g.plane; i += gridDim.x * blockDim.x)
    x[i] = defect_value(x[i], md, stats + 3 * p, d.contrast_scale, fin);
}

// the z pass over the K sections of the draw, S planes apart: whole rows, one tap per section read
__global__ __launch_bounds__(256) void aug2d_smooth_z_kernel(Batch g, const bsmi_aug2d_idraw* __restrict__ idraws, const float* __restrict__ taps,
                                                             const float* __restrict__ in, float* __restrict__ out) {
  int k;
  const bsmi_aug2d_idraw d = draw_of(g, idraws, &k);
  if (!(d.nodes & BSMI_AUG2D_SMOOTH)) return;
  const int s = (int)blockIdx.y - k * g.S, r = d.radius;
  const float* __restrict__ w = taps + d.taps_offset;
  float* __restrict__ o = out + (size_t)blockIdx.y * g.plane;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < g.plane; i += gridDim.x * blockDim.x)
    o[i] = tap_sum(r, w, [&](int j) { return in[((size_t)reflect(k + j - r, g.K) * g.S + s) * g.plane + i]; });
}

// grid.z: the plane
__global__ __launch_bounds__(256) void aug2d_smooth_yx_kernel(Batch g, const bsmi_aug2d_idraw* __restrict__ idraws, const float* __restrict__ taps,
                                                              const float* __restrict__ in, float* __restrict__ out) {
  const int p = (int)blockIdx.z;
  const bsmi_aug2d_idraw d = idraws[p % g.S];
  if (!(d.nodes & BSMI_AUG2D_SMOOTH)) return;
  const size_t sec = (size_t)p * g.plane;
  smooth_yx_tile(g.H, g.W, d.radius, taps + d.taps_offset, in + sec, out + sec);
}

constexpr int kAllNodes = 127;

// the table and the batch's shape; *any: whether some draw has a bit of `node`
int check_batch(const bsmi_aug2d_idraw* idraws, const void* idraws_dev, int S, int K, const int64_t shape[2], const void* x_dev, int node, Batch* g,
                bool* any) {
  if (!idraws || !idraws_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null descriptor table");
  if (S < 1) BSMI_FAIL(BSMI_ERR_INVALID, "%d draws: at least 1", S);
  if (K < 1) BSMI_FAIL(BSMI_ERR_INVALID, "%d sections: at least 1", K);
  if ((int64_t)S * K > 65535) BSMI_FAIL(BSMI_ERR_INVALID, "%d draws of %d sections: at most 65535 planes", S, K);
  if (!shape || !x_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  for (int a = 0; a < 2; ++a)
    if (shape[a] < 1 || shape[a] > (1 << 20)) BSMI_FAIL(BSMI_ERR_INVALID, "section: shape out of range on axis %d", a);
  if ((unsigned __int128)shape[0] * shape[1] * S * K >= (1ull << 31)) BSMI_FAIL(BSMI_ERR_INVALID, "batch: 2^31 voxels or more");
  *any = false;
  for (int s = 0; s < S; ++s) {
    const bsmi_aug2d_idraw& d = idraws[s];
    if (d.nodes < 0 || d.nodes > kAllNodes) BSMI_FAIL(BSMI_ERR_INVALID, "draw %d: nodes %d: a mask of bits 0..6", s, d.nodes);
    if (d.radius < 0 || d.radius > kMaxRadius) BSMI_FAIL(BSMI_ERR_INVALID, "draw %d: smoothing radius %d: 0 .. %d", s, d.radius, kMaxRadius);
    if (d.impulse_threshold > (1ull << 32)) BSMI_FAIL(BSMI_ERR_INVALID, "draw %d: impulse threshold above 2^32", s);
    if ((d.nodes & BSMI_AUG2D_NOISE) && (!(d.noise_sigma >= 0.0f) || !(d.noise_sigma < 1e6f)))
      BSMI_FAIL(BSMI_ERR_INVALID, "draw %d: noise sigma must be finite and not negative", s);
    if (d.nodes & node) *any = true;
  }
  *g = Batch{S, K, (int)shape[0], (int)shape[1], (uint32_t)(shape[0] * shape[1])};
  return BSMI_OK;
}

dim3 grid_of(const Batch& g) { return dim3((unsigned)std::min<uint32_t>((g.plane + 255) / 256, 1024), (unsigned)(g.S * g.K)); }

}  // namespace
}  // namespace bsmi

using namespace bsmi;

extern "C" {

int bsmi_aug2d_noise_f32(int device, const bsmi_aug2d_idraw* idraws, const bsmi_aug2d_idraw* idraws_dev, int S, int K, const int64_t shape[2],
                         float* x_dev, void* stream) {
  Batch g;
  bool any;
  if (int rc = check_batch(idraws, idraws_dev, S, K, shape, x_dev, BSMI_AUG2D_NOISE, &g, &any)) return rc;
  if (!any) return BSMI_OK;
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(aug2d_noise_kernel, grid_of(g), dim3(256), 0, (hipStream_t)stream, g, idraws_dev, x_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_aug2d_impulse_f32(int device, const bsmi_aug2d_idraw* idraws, const bsmi_aug2d_idraw* idraws_dev, int S, int K, const int64_t shape[2],
                           float* x_dev, void* stream) {
  Batch g;
  bool any;
  if (int rc = check_batch(idraws, idraws_dev, S, K, shape, x_dev, BSMI_AUG2D_IMPULSE, &g, &any)) return rc;
  if (!any) return BSMI_OK;
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(aug2d_impulse_kernel, grid_of(g), dim3(256), 0, (hipStream_t)stream, g, idraws_dev, x_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_aug2d_intensity_f32(int device, const bsmi_aug2d_idraw* idraws, const bsmi_aug2d_idraw* idraws_dev, int S, int K,
                             const int64_t shape[2], float* x_dev, const float* stats_dev, const float* scale_dev, const float* shift_dev,
                             void* stream) {
  Batch g;
  bool any;
  if (int rc = check_batch(idraws, idraws_dev, S, K, shape, x_dev, BSMI_AUG2D_INTENSITY, &g, &any)) return rc;
  if (!any) return BSMI_OK;
  if (!stats_dev || !scale_dev || !shift_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(aug2d_intensity_kernel, grid_of(g), dim3(256), 0, (hipStream_t)stream, g, idraws_dev, x_dev, stats_dev, scale_dev, shift_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_aug2d_gamma_f32(int device, const bsmi_aug2d_idraw* idraws, const bsmi_aug2d_idraw* idraws_dev, int S, int K, const int64_t shape[2],
                         float* x_dev, const float* stats_dev, const float* gamma_dev, void* stream) {
  Batch g;
  bool any;
  if (int rc = check_batch(idraws, idraws_dev, S, K, shape, x_dev, BSMI_AUG2D_GAMMA, &g, &any)) return rc;
  if (!any) return BSMI_OK;
  if (!stats_dev || !gamma_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(aug2d_gamma_kernel, grid_of(g), dim3(256), 0, (hipStream_t)stream, g, idraws_dev, x_dev, stats_dev, gamma_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_aug2d_smooth_f32(int device, const bsmi_aug2d_idraw* idraws, const bsmi_aug2d_idraw* idraws_dev, int S, int K, const int64_t shape[2],
                          float* x_dev, float* tmp_dev, const float* taps_dev, int64_t taps_floats, void* stream) {
  Batch g;
  bool any;
  if (int rc = check_batch(idraws, idraws_dev, S, K, shape, x_dev, BSMI_AUG2D_SMOOTH, &g, &any)) return rc;
  if (taps_floats < 0 || taps_floats >= (1ll << 31)) BSMI_FAIL(BSMI_ERR_INVALID, "packed taps of %lld floats", (long long)taps_floats);
  for (int s = 0; s < S; ++s) {
    const bsmi_aug2d_idraw& d = idraws[s];
    if ((d.nodes & BSMI_AUG2D_SMOOTH) && (d.taps_offset < 0 || (int64_t)d.taps_offset + 2 * d.radius + 1 > taps_floats))
      BSMI_FAIL(BSMI_ERR_INVALID, "draw %d: %d taps at float %d leave the packed taps (%lld floats)", s, 2 * d.radius + 1, d.taps_offset,
                (long long)taps_floats);
  }
  if (!any) return BSMI_OK;
  if (!tmp_dev || !taps_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  const unsigned gy = (unsigned)((g.H + kTileY - 1) / kTileY);
  if (gy > 65535) BSMI_FAIL(BSMI_ERR_INVALID, "section: more than %d rows", 65535 * kTileY);
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(aug2d_smooth_z_kernel, grid_of(g), dim3(256), 0, (hipStream_t)stream, g, idraws_dev, taps_dev, x_dev, tmp_dev);
  BSMI_HIP(hipGetLastError());
  hipLaunchKernelGGL(aug2d_smooth_yx_kernel, dim3((unsigned)((g.W + kTileX - 1) / kTileX), gy, (unsigned)(S * K)), dim3(256), 0, (hipStream_t)stream,
                     g, idraws_dev, taps_dev, tmp_dev, x_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_aug2d_defect_f32(int device, const bsmi_aug2d_idraw* idraws, const bsmi_aug2d_idraw* idraws_dev, int S, int K, const int64_t shape[2],
                          float* x_dev, const float* stats_dev, const int32_t* mode, const int32_t* mode_dev, int final_map, void* stream) {
  Batch g;
  bool any;
  if (int rc = check_batch(idraws, idraws_dev, S, K, shape, x_dev, BSMI_AUG2D_DEFECT | (final_map ? BSMI_AUG2D_TOUCHED : 0), &g, &any)) return rc;
  bool low = false;
  for (int s = 0; s < S; ++s) {
    if (!(idraws[s].nodes & BSMI_AUG2D_DEFECT)) continue;
    if (!mode || !mode_dev) BSMI_FAIL(BSMI_ERR_INVALID, "draw %d has a defect and there is no mode table", s);
    for (int k = 0; k < K; ++k) {
      const int32_t md = mode[k * S + s];
      if (md < 0 || md > 3) BSMI_FAIL(BSMI_ERR_INVALID, "draw %d, section %d: defect mode %d: 0 .. 3", s, k, md);
      low |= md == 3;
    }
  }
  if (low && !stats_dev) BSMI_FAIL(BSMI_ERR_INVALID, "a low-contrast section and no statistics");
  if (!any) return BSMI_OK;
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(aug2d_defect_kernel, grid_of(g), dim3(256), 0, (hipStream_t)stream, g, idraws_dev, x_dev, stats_dev, mode_dev, final_map ? 1 : 0);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

}  // extern "C"

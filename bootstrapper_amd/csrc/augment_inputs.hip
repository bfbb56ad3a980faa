// Input augmentation of the second-stage setups (include/bsmi.h, "training augmentation of the second-stage inputs"; the rules
// in full: DESIGN.md section 7n, tests/augin_ref.py): the degradation models/3d_affs_from_*/train.py lays over the inputs made
// from synthetic labels -- NoiseAugment, IntensityAugment per channel, IntensityAugment per section, SmoothAugment per section
// and DefectAugment's low contrast -- on one float32 array [C][D][H][W] in [0, 1], changed in place.  The per-voxel arithmetic
// is that of the intensity chain of raw, the same device code (augment_intensity.h); what is new is the fourth axis: means over
// a channel and over a section across channels, parameters indexed by channel or by section, and a smoothing whose taps differ
// per section and that also runs along c.  Plane p = c D + z is H W contiguous floats: grid.y (grid.z of the tile pass) runs
// over the planes, lanes along x.  Noise is bsmi_aug_noise_f32 on the array taken as [C D][H][W] and has no kernel here.
#include "common.h"
#include "augment_intensity.h"

namespace bsmi {
namespace {

using namespace augi;

constexpr int kMaxChannels = BSMI_AUGIN_MAX_CHANNELS;
constexpr int kTapRow = 2 * kMaxRadius + 1;   // floats per section in the table of taps

struct Array {
  int C, D, H, W;
  uint32_t plane;   // H * W; C * D * plane < 2^31
};

// mean[g] = (sum of the plane means of group g, in index order) / (number of planes): axis 0 the channel g over its D
// sections, axis 1 the section g over its C channels.  stats: [C D][3] of bsmi_aug_section_stats_f32, the mean first.
__global__ __launch_bounds__(64) void augin_group_mean_kernel(int C, int D, int axis, const float* __restrict__ stats, float* __restrict__ mean) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const int groups = axis == 0 ? C : D, n = axis == 0 ? D : C;
  if (g >= groups) return;
  float s = 0.0f;
  for (int i = 0; i < n; ++i) s += stats[3 * (size_t)(axis == 0 ? g * D + i : i * D + g)];
  mean[g] = s / (float)n;
}

// x = clip(m_g + (x - m_g) * scale_g + shift_g), g the plane's channel (axis 0) or section (axis 1)
__global__ __launch_bounds__(256) void augin_intensity_kernel(Array a, int axis, float* __restrict__ xb, const float* __restrict__ mean,
                                                              const float* __restrict__ scale, const float* __restrict__ shift) {
  const int p = (int)blockIdx.y, c = p / a.D;
  const int g = axis == 0 ? c : p - c * a.D;
  float* __restrict__ x = xb + (size_t)p * a.plane;
  const float m = mean[g], sc = scale[g], sh = shift[g];
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.plane; i += gridDim.x * blockDim.x) x[i] = intensity_value(x[i], m, sc, sh);
}

// x = m_z + (x - m_z) * contrast_scale in the sections of mode 3; every other section is not touched
__global__ __launch_bounds__(256) void augin_contrast_kernel(Array a, float* __restrict__ xb, const float* __restrict__ mean,
                                                             const int32_t* __restrict__ mode, float contrast_scale) {
  const int p = (int)blockIdx.y, z = p % a.D;
  if (mode[z] != 3) return;
  float* __restrict__ x = xb + (size_t)p * a.plane;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.plane; i += gridDim.x * blockDim.x)
    x[i] = defect_value(x[i], 3, mean + z, contrast_scale, 0);
}

// the section's radius, held to what the taps' table and the LDS tiles have room for
__device__ __forceinline__ int radius_of(const int32_t* __restrict__ radius, int z) { return min(max(radius[z], 0), kMaxRadius); }

// The c pass of section blockIdx.y, in -> out.  A thread holds the C values of its column (z, y, x) in a column of LDS of its
// own -- the tap's channel reflect(c + k - r, C) is a run-time index, which a register array would answer with a scratch
// segment; lane t reads word [j][t], so a wave's access is 64 consecutive banks whatever j is.  With channels = 0 the pass is
// the identity (a copy: the tile pass cannot run in place).  A section of radius 0 is skipped by both passes.
__global__ __launch_bounds__(256) void augin_smooth_c_kernel(Array a, int channels, const float* __restrict__ weights,
                                                             const int32_t* __restrict__ radius, const float* __restrict__ in,
                                                             float* __restrict__ out) {
  __shared__ float col[kMaxChannels][256];
  const int z = (int)blockIdx.y, r = radius_of(radius, z);
  if (r == 0) return;
  const float* __restrict__ w = weights + (size_t)z * kTapRow;
  const size_t step = (size_t)a.D * a.plane;   // from a channel to the next
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.plane; i += gridDim.x * blockDim.x) {
    const size_t at0 = (size_t)z * a.plane + i;
    if (!channels) {
      for (int c = 0; c < a.C; ++c) out[at0 + c * step] = in[at0 + c * step];
      continue;
    }
    for (int c = 0; c < a.C; ++c) col[c][threadIdx.x] = in[at0 + c * step];
    for (int c = 0; c < a.C; ++c) out[at0 + c * step] = tap_sum(r, w, [&](int k) { return col[reflect(c + k - r, a.C)][threadIdx.x]; });
  }
}

// the y and x passes of plane blockIdx.z with its section's own radius and taps, from a tile staged with its halo in LDS; the
// result is held to [0, 1], so that inputs in [0, 1] stay there whatever a few ulp of the float32 taps add up to
__global__ __launch_bounds__(256) void augin_smooth_yx_kernel(Array a, const float* __restrict__ weights, const int32_t* __restrict__ radius,
                                                              const float* __restrict__ in, float* __restrict__ out) {
  const int p = (int)blockIdx.z, z = p % a.D, r = radius_of(radius, z);
  if (r == 0) return;
  const size_t sec = (size_t)p * a.plane;
  smooth_yx_tile<true>(a.H, a.W, r, weights + (size_t)z * kTapRow, in + sec, out + sec);
}

int array_of(const int64_t shape[4], Array* a) {
  if (!shape) BSMI_FAIL(BSMI_ERR_INVALID, "null shape");
  for (int d = 0; d < 4; ++d)
    if (shape[d] < 1 || shape[d] > (1 << 20)) BSMI_FAIL(BSMI_ERR_INVALID, "array: shape out of range on axis %d", d);
  if ((unsigned __int128)shape[0] * shape[1] * shape[2] * shape[3] >= (1ull << 31)) BSMI_FAIL(BSMI_ERR_INVALID, "array: 2^31 voxels or more");
  if (shape[0] * shape[1] > 65535) BSMI_FAIL(BSMI_ERR_INVALID, "array: more than 65535 planes (channels x sections)");
  *a = Array{(int)shape[0], (int)shape[1], (int)shape[2], (int)shape[3], (uint32_t)(shape[2] * shape[3])};
  return BSMI_OK;
}

int axis_of(int axis) {
  if (axis != 0 && axis != 1) BSMI_FAIL(BSMI_ERR_INVALID, "axis %d: 0 (per channel) or 1 (per section)", axis);
  return BSMI_OK;
}

dim3 grid_of(const Array& a) { return dim3((unsigned)std::min<uint32_t>((a.plane + 255) / 256, 1024), (unsigned)(a.C * a.D)); }

}  // namespace
}  // namespace bsmi

using namespace bsmi;

extern "C" {

int bsmi_augin_group_mean_f32(int device, const int64_t shape[4], const float* x_dev, float* workspace_dev, int axis, float* mean_dev, void* stream) {
  Array a;
  if (int rc = array_of(shape, &a)) return rc;
  if (int rc = axis_of(axis)) return rc;
  if (!x_dev || !workspace_dev || !mean_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  const int64_t planes[3] = {(int64_t)a.C * a.D, a.H, a.W};
  float* stats = workspace_dev + (size_t)planes[0] * BSMI_AUG_STAT_PARTS * 3;
  if (int rc = bsmi_aug_section_stats_f32(device, planes, x_dev, workspace_dev, stats, stream)) return rc;
  const int groups = axis == 0 ? a.C : a.D;
  hipLaunchKernelGGL(augin_group_mean_kernel, dim3((groups + 63) / 64), dim3(64), 0, (hipStream_t)stream, a.C, a.D, axis, stats, mean_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_augin_intensity_f32(int device, const int64_t shape[4], float* x_dev, const float* mean_dev, const float* scale_dev, const float* shift_dev,
                             int axis, void* stream) {
  Array a;
  if (int rc = array_of(shape, &a)) return rc;
  if (int rc = axis_of(axis)) return rc;
  if (!x_dev || !mean_dev || !scale_dev || !shift_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(augin_intensity_kernel, grid_of(a), dim3(256), 0, (hipStream_t)stream, a, axis, x_dev, mean_dev, scale_dev, shift_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_augin_smooth_f32(int device, const int64_t shape[4], float* x_dev, float* tmp_dev, const float* weights_dev, const int32_t* radius_dev,
                          int channels, void* stream) {
  Array a;
  if (int rc = array_of(shape, &a)) return rc;
  if (!x_dev || !tmp_dev || !weights_dev || !radius_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (channels && a.C > kMaxChannels) BSMI_FAIL(BSMI_ERR_INVALID, "smoothing along c: %d channels, at most %d", a.C, kMaxChannels);
  const unsigned gy = (unsigned)((a.H + kTileY - 1) / kTileY);
  if (gy > 65535) BSMI_FAIL(BSMI_ERR_INVALID, "array: more than %d rows", 65535 * kTileY);
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(augin_smooth_c_kernel, dim3((unsigned)std::min<uint32_t>((a.plane + 255) / 256, 1024), (unsigned)a.D), dim3(256), 0,
                     (hipStream_t)stream, a, channels ? 1 : 0, weights_dev, radius_dev, x_dev, tmp_dev);
  BSMI_HIP(hipGetLastError());
  hipLaunchKernelGGL(augin_smooth_yx_kernel, dim3((unsigned)((a.W + kTileX - 1) / kTileX), gy, (unsigned)(a.C * a.D)), dim3(256), 0,
                     (hipStream_t)stream, a, weights_dev, radius_dev, tmp_dev, x_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_augin_contrast_f32(int device, const int64_t shape[4], float* x_dev, const float* mean_dev, const int32_t* mode_dev, float contrast_scale,
                            void* stream) {
  Array a;
  if (int rc = array_of(shape, &a)) return rc;
  if (!x_dev || !mean_dev || !mode_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(augin_contrast_kernel, grid_of(a), dim3(256), 0, (hipStream_t)stream, a, x_dev, mean_dev, mode_dev, contrast_scale);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

}  // extern "C"

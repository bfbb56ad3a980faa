// The per-voxel arithmetic of the intensity augmentation, shared by the per-block launches of augment_intensity.hip and the
// batched ones of augment2d_intensity.hip: both compile these bodies, so a draw's stack through the batched chain is the
// block through the 3-D chain bit for bit (DESIGN.md sections 7k and 7m).  Device code only; include after common.h.
#pragma once
#include <stdint.h>

namespace bsmi {
namespace augi {

constexpr int kStatParts = BSMI_AUG_STAT_PARTS;   // partial reductions per section
constexpr int kMaxRadius = BSMI_AUG_MAX_RADIUS;   // of the smoothing kernel: int(4 sigma + 0.5) for sigma <= 1.5
constexpr int kTileY = 16, kTileX = 64;           // output tile of the y/x smoothing pass

// Philox4x32-10 (Salmon et al., SC'11) on the counter (c0, 0, 0, 0) with key (k0, k1)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t k0, uint32_t k1, uint32_t o[4]) {
  uint32_t a = c0, b = 0, c = 0, d = 0;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, a), lo0 = 0xD2511F53u * a;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c), lo1 = 0xCD9E8D57u * c;
    a = hi1 ^ b ^ k0;
    b = lo1;
    c = hi0 ^ d ^ k1;
    d = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  o[0] = a, o[1] = b, o[2] = c, o[3] = d;
}

__device__ __forceinline__ float clip01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// x = clip(x + sigma * n), n = sqrt(-2 ln u1) cos(2 pi u2) from words 0 and 1 of Philox on the voxel's counter
__device__ __forceinline__ float noise_value(float v, uint32_t counter, uint32_t k0, uint32_t k1, float sigma) {
  uint32_t o[4];
  philox4x32_10(counter, k0, k1, o);
  const float u1 = (float)((o[0] >> 8) + 1u) * 0x1p-24f;   // (0, 1]: exact, at most 2^24
  const float u2 = (float)(o[1] >> 8) * 0x1p-24f;          // [0, 1)
  const float n = sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
  return clip01(v + sigma * n);
}

// a voxel is replaced iff word 2 < threshold (threshold 2^32: always), by (word 3 >> 8) * 2^-24
__device__ __forceinline__ bool impulse_value(uint32_t counter, uint32_t k0, uint32_t k1, uint64_t threshold, float* v) {
  uint32_t o[4];
  philox4x32_10(counter, k0, k1, o);
  if (!((uint64_t)o[2] < threshold)) return false;
  *v = (float)(o[3] >> 8) * 0x1p-24f;
  return true;
}

// x = clip(m + (x - m) * scale + shift)
__device__ __forceinline__ float intensity_value(float v, float m, float scale, float shift) { return clip01(m + (v - m) * scale + shift); }

// x = ((x - a) / range)^g range + a with range = b - a > 1e-3 (the caller's test); the base 0 (x = a) gives a, and the result
// is held to [a, b], which the exact expression never leaves
__device__ __forceinline__ float gamma_value(float v, float a, float b, float range, float g) {
  const float t = (v - a) / range;
  const float p = t > 0.0f ? powf(t, g) : 0.0f;
  return fminf(fmaxf(p * range + a, a), b);
}

// md 0 unchanged, 1 / 2 the value becomes 0 / 1, 3 x = m + (x - m) * contrast_scale (stats read only then); then 2 x - 1 if final_map
__device__ __forceinline__ float defect_value(float v, int md, const float* __restrict__ stats3, float contrast_scale, int final_map) {
  if (md == 1) v = 0.0f;
  else if (md == 2) v = 1.0f;
  else if (md == 3) {
    const float m = stats3[0];
    v = m + (v - m) * contrast_scale;
  }
  return final_map ? 2.0f * v - 1.0f : v;
}

// scipy's "reflect" (d c b a | a b c d), repeated as often as needed: period 2 n
__device__ __forceinline__ int reflect(int i, int n) {
  const int p = 2 * n;
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - 1 - i;
}

// a tap sum "from tap 0 upwards": acc = 0, then acc += w[k] * at(k) for k = 0 .. 2 radius
template <class W, class At>
__device__ __forceinline__ float tap_sum(int radius, W w, At at) {
  float acc = 0.0f;
  for (int k = 0; k <= 2 * radius; ++k) acc += w[k] * at(k);
  return acc;
}

// The y and x passes of one kTileY x kTileX output tile of the plane `sec` (H x W), staged with its halo in LDS: y into `mid`
// (halo columns included), x out of it into `dst` (the same plane of the output).  256 threads; w: 2 r + 1 taps.  kClip holds
// the result to [0, 1], which the exact sum never leaves (the float32 taps can add up to 1 and a few ulp).
template <bool kClip = false, class W>
__device__ __forceinline__ void smooth_yx_tile(int H, int W_, int r, W w, const float* __restrict__ sec, float* __restrict__ dst) {
  constexpr int kCols = kTileX + 2 * kMaxRadius + 1;   // + 1: rows start on different banks
  __shared__ float tile[kTileY + 2 * kMaxRadius][kCols];
  __shared__ float mid[kTileY][kCols];
  const int cols = kTileX + 2 * r, rows = kTileY + 2 * r;
  const int x0 = blockIdx.x * kTileX, y0 = blockIdx.y * kTileY;
  for (int i = threadIdx.x; i < rows * cols; i += 256) {
    const int ly = i / cols, lx = i - ly * cols;
    tile[ly][lx] = sec[(size_t)reflect(y0 + ly - r, H) * W_ + reflect(x0 + lx - r, W_)];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kTileY * cols; i += 256) {
    const int ly = i / cols, lx = i - ly * cols;
    mid[ly][lx] = tap_sum(r, w, [&](int k) { return tile[ly + k][lx]; });
  }
  __syncthreads();
  const int tx = threadIdx.x % kTileX, x = x0 + tx;
  if (x >= W_) return;
  for (int ly = threadIdx.x / kTileX; ly < kTileY && y0 + ly < H; ly += 256 / kTileX) {
    const float v = tap_sum(r, w, [&](int k) { return mid[ly][tx + k]; });
    dst[(size_t)(y0 + ly) * W_ + x] = kClip ? clip01(v) : v;
  }
}

}  // namespace augi
}  // namespace bsmi

// Training targets on the device: affinities (GrowBoundary -> AddAffinities -> BalanceLabels) of one block or of the output
// ROI of a batch of samples, and 3-D local shape descriptors.  The entry points take a device, not a bsmi_unet, and share
// nothing with the training engine (train_internal.h); the 2-D setups' descriptors are in train2d.hip.
#include <cmath>
#include <vector>

#include "common.h"
#include "dev_guard.h"  // last

// Scratch comes from the stream.  With BSMI_GUARD_MB set it lies between guard zones instead, and its release waits for the stream,
// reads the zones back and counts the damaged ones for bsmi_debug_check_guards() (dev_guard.hip); the kernels are the same.
#define SCRATCH_MALLOC_ASYNC(p, n, s) \
  (::bsmi::guards_on() ? ::bsmi::guarded_malloc((void**)(p), (n), __FILE__, __LINE__) : hipMallocAsync((void**)(p), (n), (s)))
#define SCRATCH_FREE_ASYNC(p, s) (::bsmi::guards_on() ? ::bsmi::guarded_free_checked((p), (s)) : hipFreeAsync((p), (s)))

namespace bsmi {

// ---- affinity training targets (GrowBoundary -> AddAffinities -> BalanceLabels) --------------------------
constexpr int kMaxNeighborhood = 16;
struct Neighborhood {
  int n;
  int off[kMaxNeighborhood][3];
};

// out[p] = labels[p] if every voxel within L1 distance `steps` of p (same section if only_xy) has p's label,
// is unknown (unl == 0) or lies outside the block; else 0.  `steps` erosions with the 6- (4-) neighbour cross =
// one erosion with that L1 ball.  An unknown voxel belongs to every label's mask (custom_grow_boundary.py:96-100):
// it survives if the known voxels of its ball carry at most one label.
__global__ void grow_boundary_kernel(const int64_t* __restrict__ labels, const uint8_t* __restrict__ unl, int64_t* __restrict__ out,
                                     int D, int H, int W, int steps, int only_xy) {
  const size_t nvox = (size_t)D * H * W;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < nvox; p += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(p % W), y = (int)((p / W) % H), z = (int)(p / ((size_t)W * H));
    const int64_t mine = labels[p];
    const bool known = !unl || unl[p];
    int64_t want = known ? mine : -1;  // -1: any one label
    bool keep = !(known && mine == 0);
    const int rz = only_xy ? 0 : steps;
    for (int dz = -rz; dz <= rz && keep; ++dz) {
      const int zz = z + dz;
      if (zz < 0 || zz >= D) continue;
      const int ry = steps - abs(dz);
      for (int dy = -ry; dy <= ry && keep; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= H) continue;
        const int rx = ry - abs(dy);
        for (int dx = -rx; dx <= rx; ++dx) {
          const int xx = x + dx;
          if (xx < 0 || xx >= W) continue;
          const size_t q = ((size_t)zz * H + yy) * W + xx;
          if (unl && !unl[q]) continue;
          const int64_t l = labels[q];
          if (want == -1) want = l;
          if (l != want || l == 0) { keep = false; break; }
        }
      }
    }
    out[p] = keep ? mine : 0;
  }
}

__global__ void affinity_targets_kernel(const int64_t* __restrict__ labels, const uint8_t* __restrict__ unl, Neighborhood nb, int D, int H,
                                        int W, float* __restrict__ affs, float* __restrict__ mask, unsigned long long* __restrict__ counts) {
  const size_t nvox = (size_t)D * H * W;
  unsigned long long n_mask = 0, n_pos = 0;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < nvox; p += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(p % W), y = (int)((p / W) % H), z = (int)(p / ((size_t)W * H));
    const int64_t a = labels[p];
    const bool known = !unl || unl[p];
    for (int e = 0; e < nb.n; ++e) {
      const int zz = z + nb.off[e][0], yy = y + nb.off[e][1], xx = x + nb.off[e][2];
      const bool inside = zz >= 0 && zz < D && yy >= 0 && yy < H && xx >= 0 && xx < W;
      float aff = 0.f, m = 0.f;
      if (inside) {
        const int64_t b = labels[((size_t)zz * H + yy) * W + xx];
        aff = (a == b && a > 0) ? 1.f : 0.f;
        m = known ? 1.f : 0.f;
      }
      affs[(size_t)e * nvox + p] = aff;
      mask[(size_t)e * nvox + p] = m;
      n_mask += m > 0.f;
      n_pos += (m > 0.f && aff > 0.f);
    }
  }
  // wave reduction, then one atomic pair per wave
  for (int o = 32; o > 0; o >>= 1) {
    n_mask += __shfl_down(n_mask, o);
    n_pos += __shfl_down(n_pos, o);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&counts[0], n_mask);
    atomicAdd(&counts[1], n_pos);
  }
}

__global__ void balance_kernel(const float* __restrict__ affs, float* __restrict__ weights, size_t total,
                               const unsigned long long* __restrict__ counts, float clip_min, float clip_max) {
  const float n_mask = fmaxf((float)counts[0], 1.f);
  float frac = (float)counts[1] / n_mask;
  frac = fminf(fmaxf(frac, clip_min), clip_max);
  const float w_pos = 1.f / (2.f * frac), w_neg = 1.f / (2.f * (1.f - frac));
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
    weights[i] = weights[i] * (affs[i] > 0.f ? w_pos : w_neg);
}

// affinities of the output ROI of label arrays grown by the neighbourhood's context (bsmi_train_affinity_targets_roi)
// blockIdx.y = sample; affs / mask [n][S][d][h][w]; counts[2 s] masked, counts[2 s + 1] masked positives of sample s
__global__ void affinity_roi_kernel(const int64_t* __restrict__ labels, const uint8_t* __restrict__ unl, Neighborhood nb, int S, int D,
                                    int H, int W, int oz, int oy, int ox, int d, int h, int w, float* __restrict__ affs, float* __restrict__ mask,
                                    unsigned long long* __restrict__ counts) {
  const int s = blockIdx.y;
  const size_t nroi = (size_t)d * h * w, nall = (size_t)S * nroi, sample = (size_t)D * H * W;
  const int64_t* lab = labels + (size_t)s * sample;
  const uint8_t* un = unl ? unl + (size_t)s * sample : nullptr;
  unsigned long long n_mask = 0, n_pos = 0;
  for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < nroi; r += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(r % w) + ox, y = (int)((r / w) % h) + oy, z = (int)(r / ((size_t)w * h)) + oz;
    const size_t p = ((size_t)z * H + y) * W + x;
    const int64_t a = lab[p];
    const bool known = !un || un[p];
    for (int e = 0; e < nb.n; ++e) {
      const int zz = z + nb.off[e][0], yy = y + nb.off[e][1], xx = x + nb.off[e][2];
      const bool inside = zz >= 0 && zz < D && yy >= 0 && yy < H && xx >= 0 && xx < W;
      float aff = 0.f, m = 0.f;
      if (inside) {
        const int64_t b = lab[((size_t)zz * H + yy) * W + xx];
        aff = (a == b && a > 0) ? 1.f : 0.f;
        m = known ? 1.f : 0.f;
      }
      const size_t o = (size_t)e * nall + (size_t)s * nroi + r;
      affs[o] = aff;
      mask[o] = m;
      n_mask += m > 0.f;
      n_pos += (m > 0.f && aff > 0.f);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    n_mask += __shfl_down(n_mask, o);
    n_pos += __shfl_down(n_pos, o);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&counts[2 * s], n_mask);
    atomicAdd(&counts[2 * s + 1], n_pos);
  }
}

__global__ void balance_roi_kernel(const float* __restrict__ affs, float* __restrict__ weights, size_t total, size_t nroi, int S,
                                   const unsigned long long* __restrict__ counts, float clip_min, float clip_max) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int s = (int)((i / nroi) % S);
    const float n_mask = fmaxf((float)counts[2 * s], 1.f);
    float frac = (float)counts[2 * s + 1] / n_mask;
    frac = fminf(fmaxf(frac, clip_min), clip_max);
    const float w_pos = 1.f / (2.f * frac), w_neg = 1.f / (2.f * (1.f - frac));
    weights[i] = weights[i] * (affs[i] > 0.f ? w_pos : w_neg);
  }
}

}  // namespace bsmi

using namespace bsmi;

extern "C" {

int bsmi_train_affinity_targets(int device, int64_t* labels_dev, const uint8_t* unlabelled_dev, const int64_t shape[3],
                                const int32_t* neighborhood, int n, int grow_steps, int only_xy, float clip_min, float clip_max,
                                float* affs_dev, float* weights_dev, void* stream) {
  if (!labels_dev || !shape || !neighborhood || !affs_dev || !weights_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (n < 1 || n > kMaxNeighborhood) BSMI_FAIL(BSMI_ERR_INVALID, "neighborhood of %d offsets (1..%d supported)", n, kMaxNeighborhood);
  if (grow_steps < 0 || grow_steps > 16) BSMI_FAIL(BSMI_ERR_INVALID, "grow_steps %d outside 0..16", grow_steps);
  for (int d = 0; d < 3; ++d)
    if (shape[d] < 1 || shape[d] > 4096) BSMI_FAIL(BSMI_ERR_INVALID, "bad shape");
  BSMI_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const int D = (int)shape[0], H = (int)shape[1], W = (int)shape[2];
  const size_t nvox = (size_t)D * H * W;
  Neighborhood nb;
  nb.n = n;
  for (int e = 0; e < n; ++e)
    for (int d = 0; d < 3; ++d) nb.off[e][d] = neighborhood[3 * e + d];
  // scratch on the stream: the grown labels (the erosion reads its neighbours' old values) and two counters
  int64_t* grown = nullptr;
  unsigned long long* counts = nullptr;
  BSMI_HIP(SCRATCH_MALLOC_ASYNC(&grown, nvox * sizeof(int64_t) + 2 * sizeof(unsigned long long), s));
  counts = (unsigned long long*)(grown + nvox);
  BSMI_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(unsigned long long), s));
  const int bs = 256;
  const unsigned grid = (unsigned)std::min<size_t>((nvox + bs - 1) / bs, 65535);
  hipLaunchKernelGGL(grow_boundary_kernel, dim3(grid), dim3(bs), 0, s, labels_dev, unlabelled_dev, grown, D, H, W, grow_steps, only_xy);
  BSMI_HIP(hipMemcpyAsync(labels_dev, grown, nvox * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(affinity_targets_kernel, dim3(grid), dim3(bs), 0, s, grown, unlabelled_dev, nb, D, H, W, affs_dev, weights_dev, counts);
  const size_t total = nvox * (size_t)n;
  hipLaunchKernelGGL(balance_kernel, dim3((unsigned)std::min<size_t>((total + bs - 1) / bs, 65535)), dim3(bs), 0, s, affs_dev, weights_dev, total,
                     counts, clip_min, clip_max);
  BSMI_HIP(hipGetLastError());
  BSMI_HIP(SCRATCH_FREE_ASYNC(grown, s));
  return BSMI_OK;
}

int bsmi_train_affinity_targets_roi(int device, int64_t* labels_dev, const uint8_t* unlabelled_dev, int n_samples, const int64_t shape[3],
                                    const int64_t roi_offset[3], const int64_t roi_shape[3], const int32_t* neighborhood, int n,
                                    int grow_steps, int only_xy, float clip_min, float clip_max, float* affs_dev, float* weights_dev,
                                    void* stream) {
  if (!labels_dev || !shape || !roi_offset || !roi_shape || !neighborhood || !affs_dev || !weights_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (n < 1 || n > kMaxNeighborhood) BSMI_FAIL(BSMI_ERR_INVALID, "neighborhood of %d offsets (1..%d supported)", n, kMaxNeighborhood);
  if (grow_steps < 0 || grow_steps > 16) BSMI_FAIL(BSMI_ERR_INVALID, "grow_steps %d outside 0..16", grow_steps);
  if (n_samples < 1 || n_samples > 65535) BSMI_FAIL(BSMI_ERR_INVALID, "n_samples %d outside 1..65535", n_samples);
  for (int d = 0; d < 3; ++d) {
    if (shape[d] < 1 || shape[d] > 65536) BSMI_FAIL(BSMI_ERR_INVALID, "bad shape");
    if (roi_shape[d] < 1 || roi_offset[d] < 0 || roi_offset[d] + roi_shape[d] > shape[d]) BSMI_FAIL(BSMI_ERR_INVALID, "ROI outside the label array");
  }
  const int S = n_samples, D = (int)shape[0], H = (int)shape[1], W = (int)shape[2];
  const size_t nvox = (size_t)S * D * H * W, nroi = (size_t)roi_shape[0] * roi_shape[1] * roi_shape[2];
  if (nvox > ((size_t)1 << 40) || (int64_t)S * D > INT32_MAX) BSMI_FAIL(BSMI_ERR_INVALID, "bad shape");
  Neighborhood nb;
  nb.n = n;
  for (int e = 0; e < n; ++e)
    for (int d = 0; d < 3; ++d) nb.off[e][d] = neighborhood[3 * e + d];
  BSMI_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  // scratch on the stream: the grown labels (the erosion reads its neighbours' old values) and two counters per sample
  int64_t* grown = nullptr;
  BSMI_HIP(SCRATCH_MALLOC_ASYNC(&grown, nvox * sizeof(int64_t) + 2 * (size_t)S * sizeof(unsigned long long), s));
  unsigned long long* counts = (unsigned long long*)(grown + nvox);
  BSMI_HIP(hipMemsetAsync(counts, 0, 2 * (size_t)S * sizeof(unsigned long long), s));
  const int bs = 256;
  const unsigned ggrid = (unsigned)std::min<size_t>((nvox + bs - 1) / bs, 65535);
  if (only_xy)  // sections never see each other: the samples' sections are one stack
    hipLaunchKernelGGL(grow_boundary_kernel, dim3(ggrid), dim3(bs), 0, s, labels_dev, unlabelled_dev, grown, S * D, H, W, grow_steps, 1);
  else
    for (int i = 0; i < S; ++i) {
      const size_t o = (size_t)i * D * H * W;
      hipLaunchKernelGGL(grow_boundary_kernel, dim3(ggrid), dim3(bs), 0, s, labels_dev + o, unlabelled_dev ? unlabelled_dev + o : nullptr,
                         grown + o, D, H, W, grow_steps, 0);
    }
  BSMI_HIP(hipMemcpyAsync(labels_dev, grown, nvox * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(affinity_roi_kernel, dim3((unsigned)std::min<size_t>((nroi + bs - 1) / bs, 4096), (unsigned)S), dim3(bs), 0, s, grown,
                     unlabelled_dev, nb, S, D, H, W, (int)roi_offset[0], (int)roi_offset[1], (int)roi_offset[2], (int)roi_shape[0],
                     (int)roi_shape[1], (int)roi_shape[2], affs_dev, weights_dev, counts);
  const size_t total = nroi * S * (size_t)n;
  hipLaunchKernelGGL(balance_roi_kernel, dim3((unsigned)std::min<size_t>((total + bs - 1) / bs, 65535)), dim3(bs), 0, s, affs_dev, weights_dev,
                     total, nroi, S, counts, clip_min, clip_max);
  BSMI_HIP(hipGetLastError());
  BSMI_HIP(SCRATCH_FREE_ASYNC(grown, s));
  return BSMI_OK;
}

// ---- local shape descriptors (3-D, 10 channels) -------------------------------------------------------------
// lsd.train.LsdExtractor.get_descriptors as AddLocalShapeDescriptor calls it (reference models/3d_mtlsd/train.py:134-141;
// the lsd package is not in /root/reference: restated from its published algorithm, see oracle/lsd_ref.py).  For a voxel p
// of object l the statistics are those of l inside a Gaussian window around p's cell of the `df`-times sub-sampled grid:
//   count = sum_t w(t - s) [label(t) == l],  mean = sum w c(t) / count,  cov = sum w c c^T / count - mean mean^T
// with s = p / df (integer), t over the sub-sampled grid, c = world coordinates of the sub-grid points and w the product
// of normalised 1-D Gaussians truncated at 3 sigma (scipy.ndimage.gaussian_filter(mode="constant", truncate=3.0)).
// Channels: mean - c(s) (z, y, x) / sigma * 0.5 + 0.5 | variances / sigma^2 | Pearson zy, zx, yx * 0.5 + 0.5 | count;
// clipped to [0, 1]; background voxels are all zero.  Coordinates are taken relative to s (the differences are what
// enters; the library's absolute float32 coordinates only add rounding).  A label with no tap in the window (count 0: an
// object thinner than df that misses the sub-sampled grid) has mean 0 in the library's absolute coordinates and covariance
// 0: its offset is minus the position of s, the variances are the 1e-3 floor, the Pearson channels 0.5.
struct LsdArgs {
  const int64_t* labels;  // [D][H][W] with the context the window needs
  int D, H, W;
  int oz, oy, ox, d, h, w;  // output ROI inside the label array
  int df;                   // sub-sampling factor
  int rz, ry, rx;           // window radii on the sub-sampled grid
  float step[3];            // world distance between sub-grid points
  float sigma[3];           // world units
  const float* wz; const float* wy; const float* wx;  // normalised 1-D weights [2r + 1]
};

__global__ void lsd_targets_kernel(LsdArgs a, const uint8_t* __restrict__ unl, float* __restrict__ lsds, float* __restrict__ weights) {
  const size_t nout = (size_t)a.d * a.h * a.w;
  const int SD = a.D / a.df, SH = a.H / a.df, SW = a.W / a.df;  // sub-sampled extent (labels[::df])
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < nout; p += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(p % a.w), y = (int)((p / a.w) % a.h), z = (int)(p / ((size_t)a.w * a.h));
    const int Z = z + a.oz, Y = y + a.oy, X = x + a.ox;
    const size_t q0 = ((size_t)Z * a.H + Y) * a.W + X;
    const int64_t l = a.labels[q0];
    float out[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (l != 0) {
      const int sz = Z / a.df, sy = Y / a.df, sx = X / a.df;
      double n = 0, m[3] = {0, 0, 0}, c[6] = {0, 0, 0, 0, 0, 0};
      for (int dz = -a.rz; dz <= a.rz; ++dz) {
        const int tz = sz + dz;
        if (tz < 0 || tz >= SD) continue;
        const float gz = a.wz[dz + a.rz];
        for (int dy = -a.ry; dy <= a.ry; ++dy) {
          const int ty = sy + dy;
          if (ty < 0 || ty >= SH) continue;
          const float gzy = gz * a.wy[dy + a.ry];
          const int64_t* row = a.labels + ((size_t)(tz * a.df) * a.H + (size_t)ty * a.df) * a.W;
          for (int dx = -a.rx; dx <= a.rx; ++dx) {
            const int tx = sx + dx;
            if (tx < 0 || tx >= SW) continue;
            if (row[(size_t)tx * a.df] != l) continue;
            const double wgt = (double)(gzy * a.wx[dx + a.rx]);
            const double cz = dz * (double)a.step[0], cy = dy * (double)a.step[1], cx = dx * (double)a.step[2];
            n += wgt;
            m[0] += wgt * cz; m[1] += wgt * cy; m[2] += wgt * cx;
            c[0] += wgt * cz * cz; c[1] += wgt * cy * cy; c[2] += wgt * cx * cx;
            c[3] += wgt * cz * cy; c[4] += wgt * cz * cx; c[5] += wgt * cy * cx;
          }
        }
      }
      const double cnt = n == 0 ? 1.0 : n;
      double mean[3], var[3], pe[3];
      for (int i = 0; i < 3; ++i) mean[i] = m[i] / cnt;
      for (int i = 0; i < 3; ++i) var[i] = c[i] / cnt - mean[i] * mean[i];
      pe[0] = c[3] / cnt - mean[0] * mean[1];
      pe[1] = c[4] / cnt - mean[0] * mean[2];
      pe[2] = c[5] / cnt - mean[1] * mean[2];
      for (int i = 0; i < 3; ++i) var[i] = var[i] < 1e-3 ? 1e-3 : var[i];
      pe[0] /= sqrt(var[0] * var[1]);
      pe[1] /= sqrt(var[0] * var[2]);
      pe[2] /= sqrt(var[1] * var[2]);
      if (n == 0) {
        // a label absent from the window gets the lsd package's values: mean 0 in absolute coordinates of the array, i.e. an
        // offset of minus the cell's position (as lsd2d_targets_kernel does); the covariance above is that of no tap: 0
        mean[0] = -(double)sz * a.step[0];
        mean[1] = -(double)sy * a.step[1];
        mean[2] = -(double)sx * a.step[2];
      }
      for (int i = 0; i < 3; ++i) {
        out[i] = (float)(mean[i] / a.sigma[i] * 0.5 + 0.5);
        out[3 + i] = (float)(var[i] / ((double)a.sigma[i] * a.sigma[i]));
        out[6 + i] = (float)(pe[i] * 0.5 + 0.5);
      }
      out[9] = (float)n;
      for (int i = 0; i < 10; ++i) out[i] = out[i] < 0.f ? 0.f : (out[i] > 1.f ? 1.f : out[i]);
    }
    // lsds_mask: labelled voxels, times the known-voxel mask (AddLocalShapeDescriptor.process)
    const float wv = (l != 0 && (!unl || unl[q0])) ? 1.f : 0.f;
    for (int i = 0; i < 10; ++i) {
      lsds[(size_t)i * nout + p] = out[i];
      if (weights) weights[(size_t)i * nout + p] = wv;
    }
  }
}

int bsmi_train_lsd_targets(int device, const int64_t* labels_dev, const uint8_t* unlabelled_dev, const int64_t shape[3],
                                      const int64_t roi_offset[3], const int64_t roi_shape[3], const float sigma[3],
                                      const float voxel_size[3], int downsample, float* lsds_dev, float* weights_dev, void* stream) {
  if (!labels_dev || !shape || !roi_offset || !roi_shape || !sigma || !voxel_size || !lsds_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (downsample < 1 || downsample > 8) BSMI_FAIL(BSMI_ERR_INVALID, "downsample %d outside 1..8", downsample);
  LsdArgs a;
  a.labels = labels_dev;
  a.D = (int)shape[0]; a.H = (int)shape[1]; a.W = (int)shape[2];
  a.oz = (int)roi_offset[0]; a.oy = (int)roi_offset[1]; a.ox = (int)roi_offset[2];
  a.d = (int)roi_shape[0]; a.h = (int)roi_shape[1]; a.w = (int)roi_shape[2];
  a.df = downsample;
  for (int i = 0; i < 3; ++i) {
    if (shape[i] < 1 || shape[i] > 4096 || roi_shape[i] < 1 || roi_offset[i] < 0 || roi_offset[i] + roi_shape[i] > shape[i])
      BSMI_FAIL(BSMI_ERR_INVALID, "bad shape / ROI");
    if (shape[i] % downsample || roi_offset[i] % downsample || roi_shape[i] % downsample)
      BSMI_FAIL(BSMI_ERR_INVALID, "shape and ROI must be multiples of the downsample factor %d (as the lsd package requires)", downsample);
    if (!(sigma[i] > 0.f) || !(voxel_size[i] > 0.f)) BSMI_FAIL(BSMI_ERR_INVALID, "sigma and voxel_size must be positive");
    a.sigma[i] = sigma[i];
    a.step[i] = voxel_size[i] * downsample;
  }
  BSMI_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  // normalised 1-D weights as scipy's gaussian_filter1d builds them (sigma in sub-grid voxels, truncate = 3.0)
  int r[3];
  std::vector<float> w[3];
  for (int i = 0; i < 3; ++i) {
    const double sv = (double)sigma[i] / ((double)voxel_size[i] * downsample);
    r[i] = (int)(3.0 * sv + 0.5);
    if (r[i] > 512) BSMI_FAIL(BSMI_ERR_INVALID, "LSD window radius %d too large", r[i]);
    std::vector<double> g(2 * r[i] + 1);
    double sum = 0;
    for (int k = -r[i]; k <= r[i]; ++k) sum += g[k + r[i]] = exp(-0.5 * (double)k * k / (sv * sv));
    w[i].resize(g.size());
    for (size_t k = 0; k < g.size(); ++k) w[i][k] = (float)(g[k] / sum);
  }
  a.rz = r[0]; a.ry = r[1]; a.rx = r[2];
  float* wdev = nullptr;
  const size_t nw = w[0].size() + w[1].size() + w[2].size();
  BSMI_HIP(SCRATCH_MALLOC_ASYNC(&wdev, nw * sizeof(float), s));
  std::vector<float> all;
  for (int i = 0; i < 3; ++i) all.insert(all.end(), w[i].begin(), w[i].end());
  // the host vector must outlive the asynchronous copy: copy synchronously (a few hundred bytes)
  BSMI_HIP(hipStreamSynchronize(s));
  BSMI_HIP(hipMemcpy(wdev, all.data(), nw * sizeof(float), hipMemcpyHostToDevice));
  a.wz = wdev; a.wy = wdev + w[0].size(); a.wx = wdev + w[0].size() + w[1].size();
  const size_t nout = (size_t)a.d * a.h * a.w;
  hipLaunchKernelGGL(lsd_targets_kernel, dim3((unsigned)std::min<size_t>((nout + 127) / 128, 65535)), dim3(128), 0, s, a, unlabelled_dev, lsds_dev,
                     weights_dev);
  BSMI_HIP(hipGetLastError());
  BSMI_HIP(SCRATCH_FREE_ASYNC(wdev, s));
  return BSMI_OK;
}

}  // extern "C"

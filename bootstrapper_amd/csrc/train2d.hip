// Training targets of the 2-D setups (reference models/2d_mtlsd/train.py:29-164, 2d_lsd, 2d_affs) for a batch of sections
// (their affinities: bsmi_train_affinity_targets_roi in train_targets.hip, beside the erosion it shares with the 3-D entry).
//
//   lsd2d_targets_kernel   Add2DLSDs (gp/add_2d_lsds.py: lsd's LsdExtractor with sigma (0, s, s), 6 channels) of S sections in
//                          one launch.  Voxels that share a sub-grid cell and a label share their statistics, so a thread owns a
//                          cell and runs the window once per distinct label of the cell (one label in all but boundary cells).
//                          A workgroup stages the sub-sampled labels of its 16 x 16 cells and their window context in LDS.
//   mask_sat_*_kernel      summed-area table of a stack of mask sections (the sample source's O(1) rejection test).
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/bsmi.h"
#include "common.h"

#include "dev_guard.h"  // last: routes hipMalloc / hipFree through the guarded allocator (BSMI_GUARD_MB)

namespace bsmi {

// ---- 2-D local shape descriptors (6 channels) ------------------------------------------------------------------------
// For a voxel p of object l in section s the statistics are those of l inside a Gaussian window around p's cell c = p / df
// of the df-times sub-sampled section (labels[::df, ::df]):
//   count = sum_t w(t - c) [label(t) == l],  mean = sum w u(t) / count,  cov = sum w (u - mean)(u - mean)^T / count
// with u = world coordinates relative to c and w the product of normalised 1-D Gaussians truncated at 3 sigma
// (scipy gaussian_filter(mode="constant", truncate=3.0)); taps beyond the array are 0.  Channels: mean (y, x) / sigma * 0.5
// + 0.5 | variances / sigma^2 | Pearson yx * 0.5 + 0.5 | count, clipped to [0, 1]; background voxels are all zero.
// f32 in two passes (mean first, then the central moments): relative coordinates are at most r * step, and centring keeps a
// window with one tap from turning rounding into a Pearson coefficient.  A label absent from the window (count 0) gets the
// lsd package's values: mean 0 in absolute coordinates of the array, i.e. an offset of minus the cell's position.
constexpr int kLsd2dTile = 16;       // cells per workgroup side, one thread each
constexpr int kLsd2dMaxRadius = 60;  // (16 + 2 * 60)^2 int64 labels = 148 KB of LDS
constexpr int kLsd2dMaxDf = 8;

struct Lsd2dArgs {
  const int64_t* labels;  // [S][H][W]: sections with the window context
  const uint8_t* unl;     // [S][H][W] or null
  float* lsds;            // [6][S][h][w]
  float* weights;         // [6][S][h][w] or null
  int S, H, W;
  int oy, ox, h, w;       // output ROI in every section
  int df, ry, rx;         // sub-sampling factor, window radii on the sub-sampled grid
  float step[2];          // world distance between sub-grid points
  float sigma[2];
  float wy[2 * kLsd2dMaxRadius + 1], wx[2 * kLsd2dMaxRadius + 1];  // normalised 1-D weights [2r + 1]
};

static size_t lsd2d_lds_bytes(int ry, int rx) {
  return (size_t)(kLsd2dTile + 2 * ry) * (kLsd2dTile + 2 * rx) * sizeof(int64_t) + (size_t)(2 * ry + 1 + 2 * (2 * rx + 1)) * sizeof(float);
}

__global__ __launch_bounds__(256) void lsd2d_targets_kernel(const Lsd2dArgs a) {
  extern __shared__ int64_t tile[];  // [LY][LX] sub-sampled labels of the workgroup's cells and their window context
  const int LY = kLsd2dTile + 2 * a.ry, LX = kLsd2dTile + 2 * a.rx;
  float* wys = (float*)(tile + LY * LX);  // [2 ry + 1]
  float* wxs = wys + 2 * a.ry + 1;        // [2 rx + 1]
  float* cxs = wxs + 2 * a.rx + 1;        // [2 rx + 1]: x of the tap relative to the cell
  const int s = blockIdx.z;
  const int SH = a.H / a.df, SW = a.W / a.df;
  const int cy0 = a.oy / a.df + blockIdx.y * kLsd2dTile, cx0 = a.ox / a.df + blockIdx.x * kLsd2dTile;
  const int64_t* lab = a.labels + (size_t)s * a.H * a.W;
  for (int i = threadIdx.x; i < LY * LX; i += blockDim.x) {
    const int ty = cy0 - a.ry + i / LX, tx = cx0 - a.rx + i % LX;
    // beyond the array: 0, which no queried label equals
    tile[i] = (ty >= 0 && ty < SH && tx >= 0 && tx < SW) ? lab[(size_t)ty * a.df * a.W + (size_t)tx * a.df] : 0;
  }
  for (int k = threadIdx.x; k <= 2 * a.ry; k += blockDim.x) wys[k] = a.wy[k];
  for (int k = threadIdx.x; k <= 2 * a.rx; k += blockDim.x) {
    wxs[k] = a.wx[k];
    cxs[k] = (float)(k - a.rx) * a.step[1];
  }
  __syncthreads();
  const int ly = threadIdx.x / kLsd2dTile, lx = threadIdx.x % kLsd2dTile;
  const int cy = cy0 + ly, cx = cx0 + lx;
  if (cy >= (a.oy + a.h) / a.df || cx >= (a.ox + a.w) / a.df) return;
  const size_t nout = (size_t)a.S * a.h * a.w;
  const int64_t* win = tile + ly * LX + lx;  // tap (dy, dx) = (-ry, -rx) of this cell's window
  const int nv = a.df * a.df;
  for (int v = 0; v < nv; ++v) {
    const int Y0 = cy * a.df + v / a.df, X0 = cx * a.df + v % a.df;
    const int64_t l = lab[(size_t)Y0 * a.W + X0];
    bool seen = false;  // an earlier voxel of the cell with this label has written it already
    for (int u = 0; u < v && !seen; ++u) seen = lab[(size_t)(cy * a.df + u / a.df) * a.W + cx * a.df + u % a.df] == l;
    if (seen) continue;
    float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f, o4 = 0.f, o5 = 0.f;
    if (l != 0) {
      float n = 0.f, my = 0.f, mx = 0.f;
      for (int j = 0; j <= 2 * a.ry; ++j) {
        const int64_t* row = win + j * LX;
        float rn = 0.f, rx = 0.f;
        for (int k = 0; k <= 2 * a.rx; ++k) {
          const float wk = row[k] == l ? wxs[k] : 0.f;
          rn += wk;
          rx = fmaf(wk, cxs[k], rx);
        }
        const float wj = wys[j], uy = (float)(j - a.ry) * a.step[0];
        n = fmaf(wj, rn, n);
        my = fmaf(wj * uy, rn, my);
        mx = fmaf(wj, rx, mx);
      }
      float vy = 0.f, vx = 0.f, cyx = 0.f;
      if (n > 0.f) {
        my /= n;
        mx /= n;
        for (int j = 0; j <= 2 * a.ry; ++j) {
          const int64_t* row = win + j * LX;
          float rn = 0.f, rd = 0.f, rdd = 0.f;
          for (int k = 0; k <= 2 * a.rx; ++k) {
            const float wk = row[k] == l ? wxs[k] : 0.f;
            const float d = cxs[k] - mx;
            rn += wk;
            rd = fmaf(wk, d, rd);
            rdd = fmaf(wk * d, d, rdd);
          }
          const float wj = wys[j], dy = (float)(j - a.ry) * a.step[0] - my;
          vy = fmaf(wj * dy * dy, rn, vy);
          vx = fmaf(wj, rdd, vx);
          cyx = fmaf(wj * dy, rd, cyx);
        }
        vy /= n;
        vx /= n;
        cyx /= n;
      } else {
        my = -(float)cy * a.step[0];
        mx = -(float)cx * a.step[1];
      }
      vy = fmaxf(vy, 1e-3f);
      vx = fmaxf(vx, 1e-3f);
      o0 = my / a.sigma[0] * 0.5f + 0.5f;
      o1 = mx / a.sigma[1] * 0.5f + 0.5f;
      o2 = vy / (a.sigma[0] * a.sigma[0]);
      o3 = vx / (a.sigma[1] * a.sigma[1]);
      o4 = cyx / sqrtf(vy * vx) * 0.5f + 0.5f;
      o5 = n;
      o0 = fminf(fmaxf(o0, 0.f), 1.f); o1 = fminf(fmaxf(o1, 0.f), 1.f); o2 = fminf(fmaxf(o2, 0.f), 1.f);
      o3 = fminf(fmaxf(o3, 0.f), 1.f); o4 = fminf(fmaxf(o4, 0.f), 1.f); o5 = fminf(fmaxf(o5, 0.f), 1.f);
    }
    for (int u = v; u < nv; ++u) {
      const int Y = cy * a.df + u / a.df, X = cx * a.df + u % a.df;
      const size_t q = (size_t)Y * a.W + X;
      if (u != v && lab[q] != l) continue;
      const size_t p = ((size_t)s * a.h + (Y - a.oy)) * a.w + (X - a.ox);
      a.lsds[p] = o0;
      a.lsds[nout + p] = o1;
      a.lsds[2 * nout + p] = o2;
      a.lsds[3 * nout + p] = o3;
      a.lsds[4 * nout + p] = o4;
      a.lsds[5 * nout + p] = o5;
      if (a.weights) {
        // lsds_mask: labelled voxels, times the known-voxel mask
        const float wv = (l != 0 && (!a.unl || a.unl[(size_t)s * a.H * a.W + q])) ? 1.f : 0.f;
        for (int c = 0; c < 6; ++c) a.weights[(size_t)c * nout + p] = wv;
      }
    }
  }
}

// ---- summed-area table of mask sections: sat[s][y][x] = #{(y', x') : y' < y, x' < x, mask[s][y'][x'] != 0} --------------
__global__ void mask_sat_rows_kernel(const uint8_t* __restrict__ mask, uint32_t* __restrict__ sat, int S, int H, int W) {
  const size_t nrows = (size_t)S * (H + 1);
  for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += (size_t)gridDim.x * blockDim.x) {
    const size_t s = r / (H + 1);
    const int y = (int)(r % (H + 1));
    uint32_t* out = sat + r * (W + 1);
    out[0] = 0;
    uint32_t acc = 0;
    const uint8_t* in = y > 0 ? mask + (s * H + (y - 1)) * (size_t)W : nullptr;  // row 0 of the table is all zeros
    for (int x = 0; x < W; ++x) {
      if (in) acc += in[x] != 0;
      out[x + 1] = acc;
    }
  }
}

__global__ void mask_sat_cols_kernel(uint32_t* __restrict__ sat, int S, int H, int W) {
  const size_t ncols = (size_t)S * (W + 1);
  for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < ncols; c += (size_t)gridDim.x * blockDim.x) {
    const size_t s = c / (W + 1), x = c % (W + 1);
    uint32_t* col = sat + s * (size_t)(H + 1) * (W + 1) + x;
    uint32_t acc = 0;
    for (int y = 1; y <= H; ++y) {
      acc += col[(size_t)y * (W + 1)];
      col[(size_t)y * (W + 1)] = acc;
    }
  }
}

}  // namespace bsmi

using namespace bsmi;

extern "C" {

int bsmi_train_lsd2d_targets(int device, const int64_t* labels_dev, const uint8_t* unlabelled_dev, int n_sections, const int64_t shape[2],
                             const int64_t roi_offset[2], const int64_t roi_shape[2], const float sigma[2], const float voxel_size[2],
                             int downsample, float* lsds_dev, float* weights_dev, void* stream) {
  if (!labels_dev || !shape || !roi_offset || !roi_shape || !sigma || !voxel_size || !lsds_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (n_sections < 1 || n_sections > 65535) BSMI_FAIL(BSMI_ERR_INVALID, "n_sections %d outside 1..65535", n_sections);
  if (downsample < 1 || downsample > kLsd2dMaxDf) BSMI_FAIL(BSMI_ERR_INVALID, "downsample %d outside 1..%d", downsample, kLsd2dMaxDf);
  Lsd2dArgs a;
  a.labels = labels_dev;
  a.unl = unlabelled_dev;
  a.lsds = lsds_dev;
  a.weights = weights_dev;
  a.S = n_sections;
  a.H = (int)shape[0]; a.W = (int)shape[1];
  a.oy = (int)roi_offset[0]; a.ox = (int)roi_offset[1];
  a.h = (int)roi_shape[0]; a.w = (int)roi_shape[1];
  a.df = downsample;
  int r[2];
  for (int i = 0; i < 2; ++i) {
    if (shape[i] < 1 || shape[i] > 65536 || roi_shape[i] < 1 || roi_offset[i] < 0 || roi_offset[i] + roi_shape[i] > shape[i])
      BSMI_FAIL(BSMI_ERR_INVALID, "bad shape / ROI");
    if (shape[i] % downsample || roi_offset[i] % downsample || roi_shape[i] % downsample)
      BSMI_FAIL(BSMI_ERR_INVALID, "shape and ROI must be multiples of the downsample factor %d (as the lsd package requires)", downsample);
    if (!(sigma[i] > 0.f) || !(voxel_size[i] > 0.f)) BSMI_FAIL(BSMI_ERR_INVALID, "sigma and voxel_size must be positive");
    a.sigma[i] = sigma[i];
    a.step[i] = voxel_size[i] * downsample;
    // normalised 1-D weights as scipy's gaussian_filter1d builds them (sigma in sub-grid voxels, truncate = 3.0)
    const double sv = (double)sigma[i] / ((double)voxel_size[i] * downsample);
    r[i] = (int)(3.0 * sv + 0.5);
    if (r[i] > kLsd2dMaxRadius)
      BSMI_FAIL(BSMI_ERR_INVALID, "LSD window radius %d too large (at most %d sub-grid points: raise downsample or lower sigma)", r[i], kLsd2dMaxRadius);
    std::vector<double> g(2 * r[i] + 1);
    double sum = 0;
    for (int k = -r[i]; k <= r[i]; ++k) sum += g[k + r[i]] = exp(-0.5 * (double)k * k / (sv * sv));
    float* dst = i == 0 ? a.wy : a.wx;
    for (int k = 0; k <= 2 * r[i]; ++k) dst[k] = (float)(g[k] / sum);
  }
  if ((size_t)n_sections * shape[0] * shape[1] > ((size_t)1 << 40)) BSMI_FAIL(BSMI_ERR_INVALID, "bad shape");
  a.ry = r[0]; a.rx = r[1];
  BSMI_HIP(hipSetDevice(device));
  const size_t lds = lsd2d_lds_bytes(a.ry, a.rx);
  static DeviceOnce once;
  int rc = once.run([&]() -> int {
    BSMI_HIP(hipFuncSetAttribute((const void*)lsd2d_targets_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lsd2d_lds_bytes(kLsd2dMaxRadius, kLsd2dMaxRadius)));
    return BSMI_OK;
  });
  if (rc) return rc;
  const dim3 grid((unsigned)ceil_div(a.w / a.df, kLsd2dTile), (unsigned)ceil_div(a.h / a.df, kLsd2dTile), (unsigned)n_sections);
  hipLaunchKernelGGL(lsd2d_targets_kernel, grid, dim3(kLsd2dTile * kLsd2dTile), lds, (hipStream_t)stream, a);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_train_mask_sat(int device, const uint8_t* mask_dev, int n_sections, int height, int width, uint32_t* sat_dev, void* stream) {
  if (!mask_dev || !sat_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (n_sections < 1 || height < 1 || width < 1 || (size_t)height * width >= ((size_t)1 << 32))
    BSMI_FAIL(BSMI_ERR_INVALID, "bad shape (%d sections of %d x %d; a section holds fewer than 2^32 voxels)", n_sections, height, width);
  BSMI_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const int bs = 256;
  const size_t nrows = (size_t)n_sections * (height + 1), ncols = (size_t)n_sections * (width + 1);
  hipLaunchKernelGGL(mask_sat_rows_kernel, dim3((unsigned)std::min<size_t>((nrows + bs - 1) / bs, 65535)), dim3(bs), 0, s, mask_dev, sat_dev,
                     n_sections, height, width);
  hipLaunchKernelGGL(mask_sat_cols_kernel, dim3((unsigned)std::min<size_t>((ncols + bs - 1) / bs, 65535)), dim3(bs), 0, s, sat_dev, n_sections,
                     height, width);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

}  // extern "C"

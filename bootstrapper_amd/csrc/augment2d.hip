// Geometric training augmentation of the 2-D setups, a whole batch per launch (include/bsmi.h, "training augmentation of
// the 2-D setups"; the rules in full: DESIGN.md section 7l, tests/aug2d_ref.py).  A step of a 2-D setup is S independent
// draws of one section each (gp.Stack(10)), every draw with its own SimpleAugment / DeformAugment / ShiftAugment plan, so
// the launches are indexed by a table of per-draw descriptors: one coordinate launch for all draws and all K adjacent
// sections (aug2d_coords_kernel), one resampling launch per array for all draws (aug2d_sample_*_kernel).  z is never
// interpolated: the map has two components, the z mirror only reorders the sections of raw.
// All of it is small and memory-bound (1.5 M coordinates at the 2d_mtlsd shape): lanes run along x, so the coordinate planes
// are read and written in whole rows; the gathers from the crops follow the map.
#include "common.h"

namespace bsmi {
namespace {

constexpr int kAug2dMaxNodes = 4096;  // 2 float planes of lattice offsets in LDS: 32 KiB per draw

struct Aug2dFrame {
  int S, K;
  int H, W;          // the input section I
  int fy, fx;        // F_lo: the frame's origin in the input section's pixels (<= 0)
  int fh, fw;        // the frame's shape
};

__device__ __forceinline__ float lerp(float a, float b, float f) { return a + f * (b - a); }

// lattice coordinate of r on one axis, q = r - F_lo (an integer): g = q * inv_sp + 1 (node 0 lies one spacing before the
// frame), clamped to the lattice; cell index and fraction
__device__ __forceinline__ void lattice_cell(float q, float inv_sp, int n, int* i0, float* f) {
  float g = q * inv_sp + 1.0f;
  g = fminf(fmaxf(g, 0.0f), (float)(n - 1));
  const int lo = min((int)g, n - 2);
  *i0 = lo;
  *f = g - (float)lo;
}

// grid.y: (draw, section); grid.x: a grid-stride walk over the frame's pixels
__global__ __launch_bounds__(256) void aug2d_coords_kernel(Aug2dFrame f, const bsmi_aug2d_draw* __restrict__ draws,
                                                           const int32_t* __restrict__ shifts, const float* __restrict__ lattice,
                                                           float* __restrict__ coords) {
  extern __shared__ float lat[];  // [2][ny][nx] of this draw
  const int s = (int)blockIdx.y / f.K, k = (int)blockIdx.y - s * f.K;
  const bsmi_aug2d_draw d = draws[s];
  const int ny = d.n[0], nx = d.n[1], nodes = ny * nx;
  for (int i = threadIdx.x; i < 2 * nodes; i += blockDim.x) lat[i] = lattice[d.lattice_offset + i];
  __syncthreads();
  const int shy = shifts ? shifts[(s * 2 + 0) * f.K + k] : 0;
  const int shx = shifts ? shifts[(s * 2 + 1) * f.K + k] : 0;
  const float cy = 0.5f * (float)(f.H - 1), cx = 0.5f * (float)(f.W - 1);  // exact: half-integers below 2^20
  const uint32_t fp = (uint32_t)f.fh * f.fw;
  float* __restrict__ py = coords + (size_t)blockIdx.y * 2 * fp;
  float* __restrict__ px = py + fp;
  const bool my = d.flags & 2, mx = d.flags & 4, swap = d.flags & 8;
  for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < fp; idx += gridDim.x * blockDim.x) {
    const int x = (int)(idx % f.fw), y = (int)(idx / f.fw);
    const int qy = y + shy, qx = x + shx;  // r - F_lo
    const float dy = (float)(qy + f.fy) - cy, dx = (float)(qx + f.fx) - cx;
    float ty = d.a[0] * dy + d.a[1] * dx;
    float tx = d.a[2] * dy + d.a[3] * dx;
    if (nodes) {
      int y0, x0;
      float wy, wx;
      lattice_cell((float)qy, d.inv_spacing[0], ny, &y0, &wy);
      lattice_cell((float)qx, d.inv_spacing[1], nx, &x0, &wx);
      const float* v = lat + y0 * nx + x0;
      ty += lerp(lerp(v[0], v[1], wx), lerp(v[nx], v[nx + 1], wx), wy);
      v += nodes;
      tx += lerp(lerp(v[0], v[1], wx), lerp(v[nx], v[nx + 1], wx), wy);
    }
    if (swap) {
      const float t = ty;
      ty = tx;
      tx = t;
    }
    py[idx] = d.src[0] + (my ? -ty : ty);
    px[idx] = d.src[1] + (mx ? -tx : tx);
  }
}

struct Aug2dRegion {
  int S, K;
  int fh, fw;      // the frame: rows and columns of a coordinate plane
  int oy, ox;      // region offset inside the frame
  int rh, rw;      // region (= output) shape
};

__device__ __forceinline__ int clampi(int v, int n) { return min(max(v, 0), n - 1); }

// floor(s + 1/2) clamped to [0, n): clamped as a float first, so that no coordinate (NaN included) overflows the conversion
__device__ __forceinline__ int nearest_index(float s, int n) { return (int)fminf(fmaxf(floorf(s + 0.5f), 0.0f), (float)(n - 1)); }

// nearest through the coordinates of section K / 2: grid.y is the draw, the crop of a draw is one section
template <class T>
__global__ __launch_bounds__(256) void aug2d_sample_nearest_kernel(Aug2dRegion g, const bsmi_aug2d_draw* __restrict__ draws,
                                                                   const float* __restrict__ coords, const T* __restrict__ crops,
                                                                   T* __restrict__ out) {
  const int s = (int)blockIdx.y;
  const bsmi_aug2d_draw d = draws[s];
  const int ch = d.crop[0], cw = d.crop[1];
  const uint32_t fp = (uint32_t)g.fh * g.fw, rp = (uint32_t)g.rh * g.rw;
  const float* __restrict__ py = coords + ((size_t)s * g.K + g.K / 2) * 2 * fp;
  const float* __restrict__ px = py + fp;
  const T* __restrict__ crop = crops + d.crop_offset;
  T* __restrict__ o = out + (size_t)s * rp;
  for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < rp; idx += gridDim.x * blockDim.x) {
    const int x = (int)(idx % g.rw), y = (int)(idx / g.rw);
    const uint32_t p = (uint32_t)(y + g.oy) * g.fw + (x + g.ox);
    const int iy = nearest_index(py[p], ch), ix = nearest_index(px[p], cw);
    o[idx] = crop[(size_t)iy * cw + ix];
  }
}

// bilinear on u8 in the plane of section k_src, written as (v * 2 - 255) / 255 into [K][S][rh][rw]; both cell corners clamped.
// grid.y: (draw, section); the crop of a draw is K sections.  kUnit: a draw whose intensity descriptor has BSMI_AUG2D_TOUCHED is
// written v / 255 instead (Normalize alone), what the intensity chain of augment2d_intensity.hip starts from
template <bool kUnit>
__global__ __launch_bounds__(256) void aug2d_sample_f32_u8_kernel(Aug2dRegion g, const bsmi_aug2d_draw* __restrict__ draws,
                                                                  const bsmi_aug2d_idraw* __restrict__ idraws, const float* __restrict__ coords,
                                                                  const uint8_t* __restrict__ crops, float* __restrict__ out) {
  const int s = (int)blockIdx.y / g.K, k = (int)blockIdx.y - s * g.K;
  const bsmi_aug2d_draw d = draws[s];
  bool unit = false;
  if constexpr (kUnit) unit = idraws[s].nodes & BSMI_AUG2D_TOUCHED;
  const int ch = d.crop[0], cw = d.crop[1];
  const int ks = (d.flags & 1) ? g.K - 1 - k : k;
  const uint32_t fp = (uint32_t)g.fh * g.fw, rp = (uint32_t)g.rh * g.rw;
  const float* __restrict__ py = coords + (size_t)blockIdx.y * 2 * fp;
  const float* __restrict__ px = py + fp;
  const uint8_t* __restrict__ crop = crops + ((size_t)d.crop_offset * g.K + (size_t)ks * ch * cw);
  float* __restrict__ o = out + ((size_t)k * g.S + s) * rp;
  for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < rp; idx += gridDim.x * blockDim.x) {
    const int x = (int)(idx % g.rw), y = (int)(idx / g.rw);
    const uint32_t p = (uint32_t)(y + g.oy) * g.fw + (x + g.ox);
    const float sy = py[p], sx = px[p];
    const float by = floorf(sy), bx = floorf(sx);
    const float wy = sy - by, wx = sx - bx;
    // a coordinate far outside (never from a plan: source_box2d contains the map) must not overflow the int conversion
    const int iy = (int)fminf(fmaxf(by, -2.0f), (float)ch), ix = (int)fminf(fmaxf(bx, -2.0f), (float)cw);
    const int y0 = clampi(iy, ch), y1 = clampi(iy + 1, ch);
    const int x0 = clampi(ix, cw), x1 = clampi(ix + 1, cw);
    const uint8_t* r0 = crop + (size_t)y0 * cw;
    const uint8_t* r1 = crop + (size_t)y1 * cw;
    const float v = lerp(lerp((float)r0[x0], (float)r0[x1], wx), lerp((float)r1[x0], (float)r1[x1], wx), wy);
    if (kUnit && unit)
      o[idx] = v / 255.0f;
    else
      o[idx] = (v * 2.0f - 255.0f) / 255.0f;  // on a pixel centre the numerator is exact: half an ulp of v * 2 / 255 - 1
  }
}

unsigned aug2d_grid(size_t pixels) { return (unsigned)std::min<size_t>((pixels + 1023) / 1024, 64); }  // four pixels per lane

constexpr int64_t kMaxAxis = 1 << 20;

int check_batch(const bsmi_aug2d_draw* draws, const void* draws_dev, int S, int K) {
  if (!draws || !draws_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null descriptor table");
  if (S < 1) BSMI_FAIL(BSMI_ERR_INVALID, "%d draws: at least 1", S);
  if (K < 1) BSMI_FAIL(BSMI_ERR_INVALID, "%d sections: at least 1", K);
  if ((int64_t)S * K > 65535) BSMI_FAIL(BSMI_ERR_INVALID, "%d draws of %d sections: at most 65535 (draw, section) pairs", S, K);
  return BSMI_OK;
}

int check_plane(const char* what, const int64_t shape[2], int64_t* pixels) {
  if (!shape) BSMI_FAIL(BSMI_ERR_INVALID, "%s: null shape", what);
  for (int a = 0; a < 2; ++a)
    if (shape[a] < 1 || shape[a] > kMaxAxis) BSMI_FAIL(BSMI_ERR_INVALID, "%s: shape out of range on axis %d", what, a);
  *pixels = shape[0] * shape[1];
  return BSMI_OK;
}

// the region lies in the frame, every draw's crop in the packed crops (`sections` per draw), every count below 2^31
int make_region(const bsmi_aug2d_draw* draws, const void* draws_dev, int S, int K, const int64_t frame_shape[2], const int64_t region_offset[2],
                const int64_t region_shape[2], int64_t crop_pixels, int sections, int out_sections, Aug2dRegion* g) {
  if (int rc = check_batch(draws, draws_dev, S, K)) return rc;
  int64_t fp, rp;
  if (int rc = check_plane("frame", frame_shape, &fp)) return rc;
  if (int rc = check_plane("region", region_shape, &rp)) return rc;
  if (!region_offset) BSMI_FAIL(BSMI_ERR_INVALID, "null region offset");
  for (int a = 0; a < 2; ++a)
    if (region_offset[a] < 0 || region_offset[a] + region_shape[a] > frame_shape[a])
      BSMI_FAIL(BSMI_ERR_INVALID, "region [%lld, %lld) leaves the frame (%lld) on axis %d", (long long)region_offset[a],
                (long long)(region_offset[a] + region_shape[a]), (long long)frame_shape[a], a);
  if ((unsigned __int128)fp * 2 * S * K >= (1ull << 31)) BSMI_FAIL(BSMI_ERR_INVALID, "2^31 coordinates or more");
  if ((unsigned __int128)rp * S * out_sections >= (1ull << 31)) BSMI_FAIL(BSMI_ERR_INVALID, "2^31 output elements or more");
  if (crop_pixels < 1 || crop_pixels >= (1ll << 31)) BSMI_FAIL(BSMI_ERR_INVALID, "packed crops of %lld pixels: 1 .. 2^31 - 1", (long long)crop_pixels);
  for (int s = 0; s < S; ++s) {
    const bsmi_aug2d_draw& d = draws[s];
    if (d.crop[0] < 1 || d.crop[1] < 1 || d.crop[0] > kMaxAxis || d.crop[1] > kMaxAxis || d.crop_offset < 0)
      BSMI_FAIL(BSMI_ERR_INVALID, "draw %d: crop %d x %d at pixel %d", s, d.crop[0], d.crop[1], d.crop_offset);
    if (((int64_t)d.crop_offset + (int64_t)d.crop[0] * d.crop[1]) * sections > crop_pixels)
      BSMI_FAIL(BSMI_ERR_INVALID, "draw %d: crop %d x %d (x %d sections) at pixel %d leaves the packed crops (%lld pixels)", s, d.crop[0], d.crop[1],
                sections, d.crop_offset, (long long)crop_pixels);
    if (d.flags < 0 || d.flags > 15) BSMI_FAIL(BSMI_ERR_INVALID, "draw %d: flags %d: a mask of bits 0..3", s, d.flags);
  }
  *g = Aug2dRegion{S, K, (int)frame_shape[0], (int)frame_shape[1], (int)region_offset[0], (int)region_offset[1], (int)region_shape[0],
                   (int)region_shape[1]};
  return BSMI_OK;
}

template <class T>
int sample_nearest(int device, const bsmi_aug2d_draw* draws, const bsmi_aug2d_draw* draws_dev, int S, int K, const float* coords_dev,
                   const int64_t frame_shape[2], const int64_t region_offset[2], const int64_t region_shape[2], const T* crops_dev,
                   int64_t crop_pixels, T* out_dev, void* stream) {
  if (!coords_dev || !crops_dev || !out_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  Aug2dRegion g;
  if (int rc = make_region(draws, draws_dev, S, K, frame_shape, region_offset, region_shape, crop_pixels, 1, 1, &g)) return rc;
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(aug2d_sample_nearest_kernel<T>, dim3(aug2d_grid((size_t)g.rh * g.rw), S), dim3(256), 0, (hipStream_t)stream, g, draws_dev,
                     coords_dev, crops_dev, out_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

}  // namespace
}  // namespace bsmi

using namespace bsmi;

extern "C" {

int bsmi_aug2d_coords(int device, const bsmi_aug2d_draw* draws, const bsmi_aug2d_draw* draws_dev, int S, int K, const int64_t input_shape[2],
                      const int64_t frame_offset[2], const int64_t frame_shape[2], const int32_t* shifts_dev, const float* lattice_dev,
                      int64_t lattice_floats, float* coords_dev, void* stream) {
  if (int rc = check_batch(draws, draws_dev, S, K)) return rc;
  int64_t ip, fp;
  if (int rc = check_plane("input section", input_shape, &ip)) return rc;
  if (int rc = check_plane("frame", frame_shape, &fp)) return rc;
  if (!frame_offset || !coords_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  for (int a = 0; a < 2; ++a)
    if (frame_offset[a] > 0 || frame_offset[a] < -kMaxAxis || frame_offset[a] + frame_shape[a] < input_shape[a])
      BSMI_FAIL(BSMI_ERR_INVALID, "frame [%lld, %lld) does not contain the input section (%lld) on axis %d", (long long)frame_offset[a],
                (long long)(frame_offset[a] + frame_shape[a]), (long long)input_shape[a], a);
  if ((unsigned __int128)fp * 2 * S * K >= (1ull << 31)) BSMI_FAIL(BSMI_ERR_INVALID, "2^31 coordinates or more");
  if (lattice_floats < 0 || lattice_floats >= (1ll << 31)) BSMI_FAIL(BSMI_ERR_INVALID, "packed lattice of %lld floats", (long long)lattice_floats);
  int max_nodes = 0;
  for (int s = 0; s < S; ++s) {
    const bsmi_aug2d_draw& d = draws[s];
    if (d.flags < 0 || d.flags > 15) BSMI_FAIL(BSMI_ERR_INVALID, "draw %d: flags %d: a mask of bits 0..3", s, d.flags);
    if ((d.flags & 8) && input_shape[0] != input_shape[1])
      BSMI_FAIL(BSMI_ERR_INVALID, "draw %d: the y/x swap needs a square input section, not %lld x %lld", s, (long long)input_shape[0],
                (long long)input_shape[1]);
    if (d.n[0] == 0 && d.n[1] == 0) continue;
    if (d.n[0] < 2 || d.n[1] < 2 || d.n[0] > kAug2dMaxNodes || d.n[1] > kAug2dMaxNodes)
      BSMI_FAIL(BSMI_ERR_INVALID, "draw %d: lattice of %d x %d nodes: 0 x 0 or at least 2 per axis", s, d.n[0], d.n[1]);
    const int nodes = d.n[0] * d.n[1];
    if (nodes > kAug2dMaxNodes)
      BSMI_FAIL(BSMI_ERR_INVALID, "draw %d: lattice of %d nodes: at most %d (32 KiB of offsets in LDS)", s, nodes, kAug2dMaxNodes);
    for (int a = 0; a < 2; ++a)
      if (!(d.inv_spacing[a] > 0.0f) || !(d.inv_spacing[a] < 1e6f))
        BSMI_FAIL(BSMI_ERR_INVALID, "draw %d: lattice spacing on axis %d must be positive", s, a);
    if (!lattice_dev || d.lattice_offset < 0 || (int64_t)d.lattice_offset + 2 * nodes > lattice_floats)
      BSMI_FAIL(BSMI_ERR_INVALID, "draw %d: lattice of %d nodes at float %d leaves the packed lattice (%lld floats)", s, nodes, d.lattice_offset,
                (long long)lattice_floats);
    max_nodes = std::max(max_nodes, nodes);
  }
  Aug2dFrame f{S, K, (int)input_shape[0], (int)input_shape[1], (int)frame_offset[0], (int)frame_offset[1], (int)frame_shape[0], (int)frame_shape[1]};
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(aug2d_coords_kernel, dim3(aug2d_grid((size_t)fp), S * K), dim3(256), (size_t)max_nodes * 2 * sizeof(float), (hipStream_t)stream,
                     f, draws_dev, shifts_dev, lattice_dev, coords_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_aug2d_sample_f32_u8(int device, const bsmi_aug2d_draw* draws, const bsmi_aug2d_draw* draws_dev, int S, int K, const float* coords_dev,
                             const int64_t frame_shape[2], const int64_t region_offset[2], const int64_t region_shape[2], const uint8_t* crops_dev,
                             int64_t crop_pixels, float* out_dev, void* stream) {
  if (!coords_dev || !crops_dev || !out_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  Aug2dRegion g;
  if (int rc = make_region(draws, draws_dev, S, K, frame_shape, region_offset, region_shape, crop_pixels, K, K, &g)) return rc;
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(aug2d_sample_f32_u8_kernel<false>, dim3(aug2d_grid((size_t)g.rh * g.rw), S * K), dim3(256), 0, (hipStream_t)stream, g, draws_dev,
                     (const bsmi_aug2d_idraw*)nullptr, coords_dev, crops_dev, out_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

// the resampling of raw stays in this translation unit with its kernel; the rest of the intensity chain is augment2d_intensity.hip
int bsmi_aug2d_sample_unit_f32_u8(int device, const bsmi_aug2d_draw* draws, const bsmi_aug2d_draw* draws_dev, const bsmi_aug2d_idraw* idraws,
                                  const bsmi_aug2d_idraw* idraws_dev, int S, int K, const float* coords_dev, const int64_t frame_shape[2],
                                  const int64_t region_offset[2], const int64_t region_shape[2], const uint8_t* crops_dev, int64_t crop_pixels,
                                  float* out_dev, void* stream) {
  if (!coords_dev || !crops_dev || !out_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  Aug2dRegion g;
  if (int rc = make_region(draws, draws_dev, S, K, frame_shape, region_offset, region_shape, crop_pixels, K, K, &g)) return rc;
  if (!idraws || !idraws_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null intensity descriptor table");
  for (int s = 0; s < S; ++s)
    if (idraws[s].nodes < 0 || idraws[s].nodes > 127) BSMI_FAIL(BSMI_ERR_INVALID, "draw %d: nodes %d: a mask of bits 0..6", s, idraws[s].nodes);
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(aug2d_sample_f32_u8_kernel<true>, dim3(aug2d_grid((size_t)g.rh * g.rw), S * K), dim3(256), 0, (hipStream_t)stream, g, draws_dev,
                     idraws_dev, coords_dev, crops_dev, out_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_aug2d_sample_nearest_i64(int device, const bsmi_aug2d_draw* draws, const bsmi_aug2d_draw* draws_dev, int S, int K, const float* coords_dev,
                                  const int64_t frame_shape[2], const int64_t region_offset[2], const int64_t region_shape[2],
                                  const int64_t* crops_dev, int64_t crop_pixels, int64_t* out_dev, void* stream) {
  return sample_nearest<int64_t>(device, draws, draws_dev, S, K, coords_dev, frame_shape, region_offset, region_shape, crops_dev, crop_pixels,
                                 out_dev, stream);
}

int bsmi_aug2d_sample_nearest_u8(int device, const bsmi_aug2d_draw* draws, const bsmi_aug2d_draw* draws_dev, int S, int K, const float* coords_dev,
                                 const int64_t frame_shape[2], const int64_t region_offset[2], const int64_t region_shape[2], const uint8_t* crops_dev,
                                 int64_t crop_pixels, uint8_t* out_dev, void* stream) {
  return sample_nearest<uint8_t>(device, draws, draws_dev, S, K, coords_dev, frame_shape, region_offset, region_shape, crops_dev, crop_pixels,
                                 out_dev, stream);
}

}  // extern "C"

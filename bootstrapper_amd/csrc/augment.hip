// Geometric training augmentation of 3-D samples (include/bsmi.h, "training augmentation"; the rules in full: DESIGN.md
// section 7j, tests/aug_ref.py).  SimpleAugment, DeformAugment and ShiftAugment compose into one coordinate map, so a
// sample costs one coordinate launch (aug_coords_kernel) and one resampling launch per array (aug_sample_*_kernel).
// Both are memory-bound and small (1.2 M voxels at the 3d_mtlsd shape): lanes run along x, so the coordinate planes are
// read and written in whole rows; the gathers from the crop follow the map and are what they are.
#include "common.h"

namespace bsmi {
namespace {

constexpr int kAugMaxNodes = 4096;  // 3 float planes of lattice offsets in LDS: 48 KiB

struct AugMap {
  int D, H, W;
  float lin[5];      // a_zz, a_yy, a_yx, a_xy, a_xx of A = u * Rz(theta)
  float centre[3];   // c = (I - 1) / 2
  float src[3];      // c_src: the block centre in voxels of the crop
  int mirror;        // bit 0 / 1 / 2: z / y / x
  int swap;          // y <-> x, applied before the mirrors
  int n[3];          // lattice nodes per axis; n[0] == 0: no elastic term
  float inv_sp[3];   // 1 / spacing
  float org[3];      // lattice coordinate of r = 0: 1 (one node before the block), 0 on a one-node axis
};

__device__ __forceinline__ float lerp(float a, float b, float f) { return a + f * (b - a); }

// lattice coordinate of r on one axis: cell index and fraction, clamped to the lattice
__device__ __forceinline__ void lattice_cell(float r, float inv_sp, float org, int n, int* i0, int* i1, float* f) {
  float g = r * inv_sp + org;
  g = fminf(fmaxf(g, 0.0f), (float)(n - 1));
  const int lo = min((int)g, max(n - 2, 0));
  *i0 = lo;
  *i1 = min(lo + 1, n - 1);
  *f = g - (float)lo;
}

__global__ __launch_bounds__(256) void aug_coords_kernel(AugMap m, const int32_t* __restrict__ shifts, const float* __restrict__ lattice,
                                                         float* __restrict__ coords) {
  extern __shared__ float lat[];  // [3][nz][ny][nx]
  const int nodes = m.n[0] * m.n[1] * m.n[2];
  for (int i = threadIdx.x; i < 3 * nodes; i += blockDim.x) lat[i] = lattice[i];
  __syncthreads();
  const uint32_t total = (uint32_t)m.D * m.H * m.W;  // fewer than 2^31 voxels
  for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const int x = (int)(idx % m.W);
    const int y = (int)(idx / m.W % m.H);
    const int z = (int)(idx / m.W / m.H);
    const float rz = (float)z;
    const float ry = (float)(y + (shifts ? shifts[z] : 0));
    const float rx = (float)(x + (shifts ? shifts[m.D + z] : 0));
    const float dz = rz - m.centre[0], dy = ry - m.centre[1], dx = rx - m.centre[2];
    float tz = m.lin[0] * dz;
    float ty = m.lin[1] * dy + m.lin[2] * dx;
    float tx = m.lin[3] * dy + m.lin[4] * dx;
    if (nodes) {
      int z0, z1, y0, y1, x0, x1;
      float fz, fy, fx;
      lattice_cell(rz, m.inv_sp[0], m.org[0], m.n[0], &z0, &z1, &fz);
      lattice_cell(ry, m.inv_sp[1], m.org[1], m.n[1], &y0, &y1, &fy);
      lattice_cell(rx, m.inv_sp[2], m.org[2], m.n[2], &x0, &x1, &fx);
      const int r00 = (z0 * m.n[1] + y0) * m.n[2], r01 = (z0 * m.n[1] + y1) * m.n[2];
      const int r10 = (z1 * m.n[1] + y0) * m.n[2], r11 = (z1 * m.n[1] + y1) * m.n[2];
      float e[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float* v = lat + a * nodes;
        const float c00 = lerp(v[r00 + x0], v[r00 + x1], fx), c01 = lerp(v[r01 + x0], v[r01 + x1], fx);
        const float c10 = lerp(v[r10 + x0], v[r10 + x1], fx), c11 = lerp(v[r11 + x0], v[r11 + x1], fx);
        e[a] = lerp(lerp(c00, c01, fy), lerp(c10, c11, fy), fz);
      }
      tz += e[0];
      ty += e[1];
      tx += e[2];
    }
    if (m.swap) {
      const float t = ty;
      ty = tx;
      tx = t;
    }
    coords[idx] = m.src[0] + ((m.mirror & 1) ? -tz : tz);
    coords[(size_t)total + idx] = m.src[1] + ((m.mirror & 2) ? -ty : ty);
    coords[2 * (size_t)total + idx] = m.src[2] + ((m.mirror & 4) ? -tx : tx);
  }
}

struct AugRegion {
  int cH, cW;          // rows and columns of the coordinate volume
  size_t plane;        // voxels of one coordinate plane
  int oz, oy, ox;      // region offset inside the coordinate volume
  int rd, rh, rw;      // region (= output) shape
  int sd, sh, sw;      // crop shape
};

__device__ __forceinline__ size_t region_voxel(const AugRegion& g, uint32_t idx) {
  const int x = (int)(idx % g.rw);
  const int y = (int)(idx / g.rw % g.rh);
  const int z = (int)(idx / g.rw / g.rh);
  return ((size_t)(z + g.oz) * g.cH + (y + g.oy)) * g.cW + (x + g.ox);
}

__device__ __forceinline__ int clampi(int v, int n) { return min(max(v, 0), n - 1); }

// floor(s + 1/2) clamped to [0, n): clamped as a float first, so that no coordinate (NaN included) overflows the conversion
__device__ __forceinline__ int nearest_index(float s, int n) { return (int)fminf(fmaxf(floorf(s + 0.5f), 0.0f), (float)(n - 1)); }

// nearest: floor(s + 1/2) per axis in float32, indices clamped to the crop
template <class T>
__global__ __launch_bounds__(256) void aug_sample_nearest_kernel(AugRegion g, const float* __restrict__ coords, const T* __restrict__ crop,
                                                                 T* __restrict__ out) {
  const uint32_t total = (uint32_t)g.rd * g.rh * g.rw;  // fewer than 2^31 voxels
  for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const size_t p = region_voxel(g, idx);
    const int z = nearest_index(coords[p], g.sd);
    const int y = nearest_index(coords[g.plane + p], g.sh);
    const int x = nearest_index(coords[2 * g.plane + p], g.sw);
    out[idx] = crop[((size_t)z * g.sh + y) * g.sw + x];
  }
}

// trilinear on u8, written as (v * 2 - 255) / 255 (Normalize + IntensityScaleShift(2, -1)); both cell corners clamped to the crop.
// kUnit: v / 255 instead (Normalize alone), what the intensity chain of augment_intensity.hip starts from
template <bool kUnit>
__global__ __launch_bounds__(256) void aug_sample_f32_u8_kernel(AugRegion g, const float* __restrict__ coords, const uint8_t* __restrict__ crop,
                                                                float* __restrict__ out) {
  const uint32_t total = (uint32_t)g.rd * g.rh * g.rw;  // fewer than 2^31 voxels
  for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const size_t p = region_voxel(g, idx);
    const float sz = coords[p], sy = coords[g.plane + p], sx = coords[2 * g.plane + p];
    const float bz = floorf(sz), by = floorf(sy), bx = floorf(sx);
    const float fz = sz - bz, fy = sy - by, fx = sx - bx;
    // a coordinate far outside (never from a plan: source_box contains the map) must not overflow the int conversion
    const int iz = (int)fminf(fmaxf(bz, -2.0f), (float)g.sd), iy = (int)fminf(fmaxf(by, -2.0f), (float)g.sh);
    const int ix = (int)fminf(fmaxf(bx, -2.0f), (float)g.sw);
    const int z0 = clampi(iz, g.sd), z1 = clampi(iz + 1, g.sd);
    const int y0 = clampi(iy, g.sh), y1 = clampi(iy + 1, g.sh);
    const int x0 = clampi(ix, g.sw), x1 = clampi(ix + 1, g.sw);
    const uint8_t* r00 = crop + ((size_t)z0 * g.sh + y0) * g.sw;
    const uint8_t* r01 = crop + ((size_t)z0 * g.sh + y1) * g.sw;
    const uint8_t* r10 = crop + ((size_t)z1 * g.sh + y0) * g.sw;
    const uint8_t* r11 = crop + ((size_t)z1 * g.sh + y1) * g.sw;
    const float c00 = lerp((float)r00[x0], (float)r00[x1], fx), c01 = lerp((float)r01[x0], (float)r01[x1], fx);
    const float c10 = lerp((float)r10[x0], (float)r10[x1], fx), c11 = lerp((float)r11[x0], (float)r11[x1], fx);
    const float v = lerp(lerp(c00, c01, fy), lerp(c10, c11, fy), fz);
    if constexpr (kUnit)
      out[idx] = v / 255.0f;
    else
      out[idx] = (v * 2.0f - 255.0f) / 255.0f;  // on a voxel centre the numerator is exact: half an ulp of v * 2 / 255 - 1
  }
}

unsigned aug_grid(size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, 2048); }

int check_dims(const char* what, const int64_t shape[3], size_t* n) {
  if (!shape) BSMI_FAIL(BSMI_ERR_INVALID, "%s: null shape", what);
  for (int d = 0; d < 3; ++d)
    if (shape[d] < 1 || shape[d] > (1 << 20)) BSMI_FAIL(BSMI_ERR_INVALID, "%s: shape out of range on axis %d", what, d);
  const unsigned __int128 v = (unsigned __int128)shape[0] * shape[1] * shape[2];
  if (v >= (1ull << 31)) BSMI_FAIL(BSMI_ERR_INVALID, "%s: 2^31 voxels or more", what);
  *n = (size_t)v;
  return BSMI_OK;
}

int make_region(const int64_t coords_shape[3], const int64_t region_offset[3], const int64_t region_shape[3], const int64_t crop_shape[3], AugRegion* g,
                size_t* n) {
  size_t plane, crop;
  if (int rc = check_dims("coordinate volume", coords_shape, &plane)) return rc;
  if (int rc = check_dims("crop", crop_shape, &crop)) return rc;
  if (int rc = check_dims("region", region_shape, n)) return rc;
  if (!region_offset) BSMI_FAIL(BSMI_ERR_INVALID, "null region offset");
  for (int d = 0; d < 3; ++d)
    if (region_offset[d] < 0 || region_offset[d] + region_shape[d] > coords_shape[d])
      BSMI_FAIL(BSMI_ERR_INVALID, "region [%lld, %lld) leaves the coordinate volume (%lld) on axis %d", (long long)region_offset[d],
                (long long)(region_offset[d] + region_shape[d]), (long long)coords_shape[d], d);
  *g = AugRegion{(int)coords_shape[1], (int)coords_shape[2], plane, (int)region_offset[0], (int)region_offset[1], (int)region_offset[2],
                 (int)region_shape[0], (int)region_shape[1], (int)region_shape[2], (int)crop_shape[0], (int)crop_shape[1], (int)crop_shape[2]};
  return BSMI_OK;
}

template <class K, class T, class U>
int sample(int device, K kernel, const float* coords_dev, const int64_t coords_shape[3], const int64_t region_offset[3], const int64_t region_shape[3],
           const T* crop_dev, const int64_t crop_shape[3], U* out_dev, void* stream) {
  if (!coords_dev || !crop_dev || !out_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  AugRegion g;
  size_t n;
  if (int rc = make_region(coords_shape, region_offset, region_shape, crop_shape, &g, &n)) return rc;
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(kernel, dim3(aug_grid(n)), dim3(256), 0, (hipStream_t)stream, g, coords_dev, crop_dev, out_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

}  // namespace
}  // namespace bsmi

using namespace bsmi;

extern "C" {

int bsmi_aug_coords(int device, const int64_t shape[3], const float linear[5], const float centre[3], const float src_centre[3], int mirror, int swap_yx,
                    const int32_t* shifts_dev, const float* lattice_dev, const int32_t lattice_shape[3], const float inv_spacing[3], float* coords_dev,
                    void* stream) {
  size_t n;
  if (int rc = check_dims("block", shape, &n)) return rc;
  if (!linear || !centre || !src_centre || !coords_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (mirror < 0 || mirror > 7) BSMI_FAIL(BSMI_ERR_INVALID, "mirror %d: a mask of bits 0..2", mirror);
  if (swap_yx && shape[1] != shape[2])
    BSMI_FAIL(BSMI_ERR_INVALID, "the y/x swap needs a square block, not %lld x %lld", (long long)shape[1], (long long)shape[2]);
  AugMap m{};
  m.D = (int)shape[0], m.H = (int)shape[1], m.W = (int)shape[2];
  for (int i = 0; i < 5; ++i) m.lin[i] = linear[i];
  for (int d = 0; d < 3; ++d) m.centre[d] = centre[d], m.src[d] = src_centre[d];
  m.mirror = mirror;
  m.swap = swap_yx ? 1 : 0;
  size_t lds = 0;
  if (lattice_dev) {
    if (!lattice_shape || !inv_spacing) BSMI_FAIL(BSMI_ERR_INVALID, "a lattice needs its shape and spacing");
    int64_t nodes = 1;
    for (int d = 0; d < 3; ++d) {
      if (lattice_shape[d] < 1 || lattice_shape[d] > kAugMaxNodes) BSMI_FAIL(BSMI_ERR_INVALID, "lattice of %d nodes on axis %d", lattice_shape[d], d);
      if (!(inv_spacing[d] > 0.0f) || !(inv_spacing[d] < 1e6f)) BSMI_FAIL(BSMI_ERR_INVALID, "lattice spacing on axis %d must be positive", d);
      nodes *= lattice_shape[d];
      m.n[d] = lattice_shape[d];
      m.inv_sp[d] = inv_spacing[d];
      m.org[d] = lattice_shape[d] > 1 ? 1.0f : 0.0f;
    }
    if (nodes > kAugMaxNodes)
      BSMI_FAIL(BSMI_ERR_INVALID, "lattice of %lld nodes: at most %d (48 KiB of offsets in LDS)", (long long)nodes, kAugMaxNodes);
    lds = (size_t)nodes * 3 * sizeof(float);
  }
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(aug_coords_kernel, dim3(aug_grid(n)), dim3(256), lds, (hipStream_t)stream, m, shifts_dev, lattice_dev, coords_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_aug_sample_f32_u8(int device, const float* coords_dev, const int64_t coords_shape[3], const int64_t region_offset[3],
                           const int64_t region_shape[3], const uint8_t* crop_dev, const int64_t crop_shape[3], float* out_dev, void* stream) {
  return sample(device, aug_sample_f32_u8_kernel<false>, coords_dev, coords_shape, region_offset, region_shape, crop_dev, crop_shape, out_dev, stream);
}

int bsmi_aug_sample_unit_f32_u8(int device, const float* coords_dev, const int64_t coords_shape[3], const int64_t region_offset[3],
                                const int64_t region_shape[3], const uint8_t* crop_dev, const int64_t crop_shape[3], float* out_dev, void* stream) {
  return sample(device, aug_sample_f32_u8_kernel<true>, coords_dev, coords_shape, region_offset, region_shape, crop_dev, crop_shape, out_dev, stream);
}

int bsmi_aug_sample_nearest_i64(int device, const float* coords_dev, const int64_t coords_shape[3], const int64_t region_offset[3],
                                const int64_t region_shape[3], const int64_t* crop_dev, const int64_t crop_shape[3], int64_t* out_dev, void* stream) {
  return sample(device, aug_sample_nearest_kernel<int64_t>, coords_dev, coords_shape, region_offset, region_shape, crop_dev, crop_shape, out_dev,
                stream);
}

int bsmi_aug_sample_nearest_u8(int device, const float* coords_dev, const int64_t coords_shape[3], const int64_t region_offset[3],
                               const int64_t region_shape[3], const uint8_t* crop_dev, const int64_t crop_shape[3], uint8_t* out_dev, void* stream) {
  return sample(device, aug_sample_nearest_kernel<uint8_t>, coords_dev, coords_shape, region_offset, region_shape, crop_dev, crop_shape, out_dev,
                stream);
}

}  // extern "C"

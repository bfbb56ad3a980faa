// Synthetic labels for the second-stage setups (3d_affs_from_*), on the device: the generator of the reference's
// gp/create_labels.py, gp/custom_grow_boundary.py (only_xy, no mask) and gp/obfuscate_labels.py, by the rules written out
// in include/bsmi.h and DESIGN.md section 7i and restated in tests/synth_ref.py.  Every random scalar is drawn on the host
// and passed in; the one draw made here is the counter hash of grow_boundary (synth_steps).
//
//   tubes    dilate: one workgroup per section, the section as bit-packed rows, both planes of the ping-pong in LDS, a
//            structuring bitmap of up to 32 x 32 as one word per row; a lane ORs shifted source words (three words of
//            the source row serve any shift below 32).
//            label: union-find over the voxels (seg_internal.h), 13 raster-preceding neighbours, roots ranked in
//            raster order by seg_labels.hip's cc_rank_roots.
//            expand: exact Euclidean feature transform, three separable passes over keys (d2 << 32 | raster index of the
//            feature); the minimum of a key is the nearest feature, the lowest raster index among equidistant ones.  A
//            pass walks outwards from its voxel and stops once the offset alone exceeds the best distance.
//   random   gaussian: three passes of 2 r + 1 taps, float32, scipy's `reflect` border repeated as often as needed.
//            argmax filter: three passes over keys (ordered value bits << 32 | ~raster index): the maximum of a key is
//            the largest value, the lowest raster index among equal ones.
//            basins: parent = best 6-neighbour if it beats the voxel, else the window argmax if that is another voxel,
//            else the voxel is a root; parents are strictly greater in key order, so every chain ends at a root.
// The volumes are small (up to 240 x 148 x 148) and every pass is one read-mostly sweep served by L2.
#include <hip/hip_runtime.h>

#include "../../include/bsmi.h"
#include "common.h"
#include "seg_internal.h"
#include "dev_guard.h"  // last: routes hipMalloc / hipFree through the guarded allocator (BSMI_GUARD_MB)

struct bsmi_synth {
  int device = 0;
  int64_t max_shape[3] = {0, 0, 0};
  size_t max_vox = 0;
  std::vector<void*> allocs;
  bsmi::FragWs frag{};         // par, rank, blk (the other fields stay null: only the cc passes run here)
  uint64_t* key_a = nullptr;   // [max_vox] keys of the separable passes; the gaussian's float planes
  uint64_t* key_b = nullptr;   // [max_vox]
  int32_t* lab_a = nullptr;    // [max_vox]
  int32_t* lab_b = nullptr;    // [max_vox]
  float* field = nullptr;      // [max_vox] squared distance field of split
  uint8_t* mask = nullptr;     // [max_vox]
  uint64_t* num_dev = nullptr; // [1] component count of the last labelling
  uint32_t* params = nullptr;  // [kParamWords] host-drawn tables of the call in flight (points, bitmaps, weights)
  uint64_t* set_keys = nullptr;  // [kSetSlots] presence table
  uint32_t* set_cnt = nullptr;   // [0] distinct ids, [1] overflow
};

namespace bsmi {
namespace {

constexpr uint64_t kNone = ~0ull;
constexpr int kMaxPoints = 4096;
constexpr int kMaxSections = 4096;
constexpr int kMaxRadius = 255;
constexpr size_t kParamWords = (size_t)kMaxSections * 35 + 3 * kMaxPoints + 2 * kMaxRadius + 1;
constexpr uint32_t kSetSlots = 1u << 16;
constexpr int kDilateLds = 64 * 1024;

__device__ __forceinline__ uint64_t kmin(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t kmax(uint64_t a, uint64_t b) { return a > b ? a : b; }

unsigned grid_for(size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, 1u << 18); }

// ---- (a) tubes ----

// grid: sections; dynamic LDS: 2 planes of H rows of `words` 32-bit words
__global__ void __launch_bounds__(256) synth_dilate_kernel(const int32_t* __restrict__ pts, int npts, const uint32_t* __restrict__ bitmaps,
                                                           const int32_t* __restrict__ bsz, const int32_t* __restrict__ iters, int H, int W,
                                                           int32_t* __restrict__ out) {
  extern __shared__ uint32_t planes[];
  const int z = blockIdx.x, words = (W + 31) >> 5, n = H * words;
  uint32_t* a = planes;
  uint32_t* b = planes + n;
  for (int i = threadIdx.x; i < n; i += 256) a[i] = 0;
  __syncthreads();
  for (int p = threadIdx.x; p < npts; p += 256)
    if (pts[3 * p] == z) atomicOr(&a[pts[3 * p + 1] * words + (pts[3 * p + 2] >> 5)], 1u << (pts[3 * p + 2] & 31));
  __syncthreads();
  const int bh = bsz[2 * z], bw = bsz[2 * z + 1], cy = bh >> 1, cx = bw >> 1;
  const uint32_t* bm = bitmaps + 32 * z;
  const uint32_t tail = (W & 31) ? (1u << (W & 31)) - 1u : ~0u;
  const int nit = iters[z];
  for (int it = 0; it < nit; ++it) {
    for (int i = threadIdx.x; i < n; i += 256) {
      const int y = i / words, w = i - y * words;
      uint32_t acc = 0;
      for (int r = 0; r < bh; ++r) {
        const int ys = y - (r - cy);
        uint32_t m = bm[r];
        if (ys < 0 || ys >= H || !m) continue;
        const uint32_t* row = a + ys * words;
        const uint32_t mid = row[w], lo = w > 0 ? row[w - 1] : 0u, hi = w + 1 < words ? row[w + 1] : 0u;
        if (!(mid | lo | hi)) continue;
        while (m) {
          const int dx = __ffs((int)m) - 1 - cx;  // out bit x takes in bit x - dx
          m &= m - 1;
          acc |= dx == 0 ? mid : (dx > 0 ? (mid << dx) | (lo >> (32 - dx)) : (mid >> -dx) | (hi << (32 + dx)));
        }
      }
      b[i] = w == words - 1 ? acc & tail : acc;
    }
    __syncthreads();
    uint32_t* t = a;
    a = b;
    b = t;
  }
  for (int i = threadIdx.x; i < H * W; i += 256) {
    const int y = i / W, x = i - y * W;
    out[((size_t)z * H + y) * W + x] = (int32_t)(a[y * words + (x >> 5)] >> (x & 31) & 1u);
  }
}

__global__ void synth_cc_init_kernel(const int32_t* __restrict__ x, size_t n, FragWs w) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) w.par[p] = x[p] ? (int32_t)p : -1;
}

// every voxel with its 13 raster-preceding neighbours of equal non-zero value (26-connectivity)
__global__ void synth_cc_union_kernel(const int32_t* __restrict__ x, int D, int H, int W, FragWs w) {
  const size_t n = (size_t)D * H * W;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const int32_t v = x[p];
    if (!v) continue;
    const int xx = (int)(p % W), y = (int)((p / W) % H), z = (int)(p / ((size_t)W * H));
    for (int dz = -1; dz <= 0; ++dz)
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          if (dz == 0 && (dy > 0 || (dy == 0 && dx >= 0))) continue;
          const int zz = z + dz, yy = y + dy, x2 = xx + dx;
          if (zz < 0 || yy < 0 || yy >= H || x2 < 0 || x2 >= W) continue;
          const size_t q = ((size_t)zz * H + yy) * W + x2;
          if (x[q] == v) cc_unite(w.par, (int)p, (int)q);
        }
  }
}

__global__ void synth_cc_write_kernel(size_t n, FragWs w, int32_t* __restrict__ out) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x)
    out[p] = w.par[p] < 0 ? 0 : w.rank[cc_find(w.par, (int)p)];
}

// feature transform, pass along x: key of the nearest non-zero voxel of the row
__global__ void synth_ft_x_kernel(const int32_t* __restrict__ lab, size_t n, int W, uint64_t* __restrict__ out) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(p % W);
    const size_t row = p - x;
    uint64_t best = kNone;
    for (int d = 0; d < W; ++d) {
      const uint64_t d2 = (uint64_t)d * d;
      if (d2 > best >> 32) break;
      if (x - d >= 0 && lab[row + x - d]) best = kmin(best, d2 << 32 | (uint64_t)(row + x - d));
      if (d && x + d < W && lab[row + x + d]) best = kmin(best, d2 << 32 | (uint64_t)(row + x + d));
    }
    out[p] = best;
  }
}

// ... along an axis of `len` positions `stride` apart, over the keys of the pass before; offsets up to maxd
__global__ void synth_ft_axis_kernel(const uint64_t* __restrict__ in, size_t n, int len, size_t stride, int maxd, uint64_t* __restrict__ out) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(p / stride % len);
    uint64_t best = kNone;
    for (int d = 0; d < len && d <= maxd; ++d) {
      const uint64_t d2 = (uint64_t)d * d;
      if (d2 > best >> 32) break;
      if (c - d >= 0) {
        const uint64_t k = in[p - (size_t)d * stride];
        if (k != kNone) best = kmin(best, k + (d2 << 32));
      }
      if (d && c + d < len) {
        const uint64_t k = in[p + (size_t)d * stride];
        if (k != kNone) best = kmin(best, k + (d2 << 32));
      }
    }
    out[p] = best;
  }
}

__global__ void synth_expand_write_kernel(const uint64_t* __restrict__ key, const int32_t* __restrict__ lab, size_t n, uint64_t depth2, int32_t fill,
                                          int32_t* __restrict__ out) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const uint64_t k = key[p];
    out[p] = (k != kNone && (k >> 32) <= depth2) ? lab[k & 0xffffffffull] : fill;
  }
}

// ---- (b) random ----

__global__ void synth_gauss_axis_kernel(const float* __restrict__ in, size_t n, int len, size_t stride, const float* __restrict__ wts, int r,
                                        float* __restrict__ out) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(p / stride % len);
    const size_t base = p - (size_t)c * stride;
    float acc = 0.f;
    for (int t = -r; t <= r; ++t) {
      const int i = c + t;
      const int j = (i < 0 || i >= len) ? reflect_dup(i, len) : i;
      acc = fmaf(wts[t + r], in[base + (size_t)j * stride], acc);
    }
    out[p] = acc;
  }
}

// total order of the field's values in the high word (-0 counts as +0), the raster index inverted in the low word: the
// larger key is the larger value, or the lower raster index among equal values
__device__ __forceinline__ uint64_t value_key(float f, size_t p) {
  uint32_t u = __float_as_uint(f + 0.0f);
  u = (u & 0x80000000u) ? ~u : u | 0x80000000u;
  return (uint64_t)u << 32 | (uint64_t)(0xffffffffu - (uint32_t)p);
}

__global__ void synth_argmax_x_kernel(const float* __restrict__ f, size_t n, int W, int lo, int hi, uint64_t* __restrict__ out) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(p % W);
    const size_t row = p - x;
    uint64_t best = 0;
    for (int t = lo; t <= hi; ++t) {
      const int i = x + t;
      const size_t q = row + ((i < 0 || i >= W) ? reflect_dup(i, W) : i);
      best = kmax(best, value_key(f[q], q));
    }
    out[p] = best;
  }
}

__global__ void synth_argmax_axis_kernel(const uint64_t* __restrict__ in, size_t n, int len, size_t stride, int lo, int hi, uint64_t* __restrict__ out) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(p / stride % len);
    const size_t base = p - (size_t)c * stride;
    uint64_t best = 0;
    for (int t = lo; t <= hi; ++t) {
      const int i = c + t;
      best = kmax(best, in[base + (size_t)((i < 0 || i >= len) ? reflect_dup(i, len) : i) * stride]);
    }
    out[p] = best;
  }
}

__global__ void synth_key_pos_kernel(const uint64_t* __restrict__ key, size_t n, int32_t* __restrict__ pos) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x)
    pos[p] = (int32_t)(0xffffffffu - (uint32_t)(key[p] & 0xffffffffull));
}

// the parent rule; a position that is no voxel of the (masked) volume or does not beat the voxel is ignored, so parents are
// strictly greater in key order whatever `pos` holds
__global__ void synth_parent_kernel(const float* __restrict__ f, const int32_t* __restrict__ pos, const uint8_t* __restrict__ mask, int D, int H, int W,
                                    FragWs w) {
  const size_t n = (size_t)D * H * W, plane = (size_t)H * W;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    if (mask && !mask[p]) {
      w.par[p] = -1;
      continue;
    }
    const int x = (int)(p % W), y = (int)((p / W) % H), z = (int)(p / plane);
    const uint64_t self = value_key(f[p], p);
    uint64_t best = self;
    auto look = [&](size_t q) {
      if (mask && !mask[q]) return;
      best = kmax(best, value_key(f[q], q));
    };
    if (z > 0) look(p - plane);
    if (y > 0) look(p - W);
    if (x > 0) look(p - 1);
    if (x + 1 < W) look(p + 1);
    if (y + 1 < H) look(p + W);
    if (z + 1 < D) look(p + plane);
    int32_t par = (int32_t)p;
    if (best != self) {
      par = (int32_t)(0xffffffffu - (uint32_t)(best & 0xffffffffull));
    } else {
      const int32_t q = pos[p];
      if (q >= 0 && (size_t)q < n && (!mask || mask[q]) && value_key(f[q], (size_t)q) > self) par = q;
    }
    w.par[p] = par;
  }
}

// root of every voxel by following the parents (read only: no lane waits for another)
__global__ void synth_root_kernel(size_t n, FragWs w, int32_t* __restrict__ root) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    int32_t a = w.par[p];
    if (a >= 0) {
      int32_t q = w.par[a];
      while (q != a) {
        a = q;
        q = w.par[a];
      }
    }
    root[p] = a;
  }
}

__global__ void synth_root_write_kernel(size_t n, FragWs w, const int32_t* __restrict__ root, int32_t* __restrict__ out) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x)
    out[p] = root[p] < 0 ? 0 : w.rank[root[p]];
}

// ---- (c) finish ----

__global__ void synth_finish_kernel(const int32_t* __restrict__ in, int H, int W, int step, int dout, int drop3, int drop5, int64_t* __restrict__ out) {
  const size_t plane = (size_t)H * W, n = plane * dout;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const size_t k = p / plane;
    int32_t v = in[k * step * plane + (p - k * plane)];
    if ((drop3 && v % 3 == 0) || (drop5 && v % 5 == 0)) v = 0;
    out[p] = v;
  }
}

// ---- (d) grow boundary ----

__device__ __forceinline__ uint32_t synth_steps(uint64_t seed, int z, uint64_t label, int max_steps) {
  return (uint32_t)(mix64(mix64(mix64(seed) ^ (uint64_t)z) ^ label) % (uint64_t)(max_steps + 1));
}

__global__ void synth_grow_kernel(const int64_t* __restrict__ in, int D, int H, int W, uint64_t seed, int max_steps, int64_t* __restrict__ out) {
  const size_t n = (size_t)D * H * W;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const int64_t l = in[p];
    int64_t keep = l;
    if (l != 0) {
      const int x = (int)(p % W), y = (int)((p / W) % H), z = (int)(p / ((size_t)W * H));
      const int s = (int)synth_steps(seed, z, (uint64_t)l, max_steps);
      for (int dy = -s; dy <= s && keep; ++dy) {
        const int yy = y + dy, r = s - (dy < 0 ? -dy : dy);
        if (yy < 0 || yy >= H) continue;
        for (int dx = -r; dx <= r; ++dx) {
          const int xx = x + dx;
          if (xx < 0 || xx >= W) continue;
          if (in[p + (int64_t)dy * W + dx] != l) {
            keep = 0;
            break;
          }
        }
      }
    }
    out[p] = keep;
  }
}

// ---- (e) obfuscate ----

struct Sections {
  int z[2];
  int n;
};
struct Bitmap {
  uint32_t row[32];
};

__global__ void synth_merge_kernel(int64_t* __restrict__ lab, int H, int W, Sections zs, int64_t a, int64_t b) {
  const size_t plane = (size_t)H * W, n = plane * zs.n;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(i / plane);
    int64_t* q = lab + (size_t)(k == 0 ? zs.z[0] : zs.z[1]) * plane + (i - k * plane);
    if (*q == b) *q = a;
  }
}

__global__ void synth_stamp_kernel(int64_t* __restrict__ lab, int H, int W, int z, int y0, int x0, Bitmap bm, int bh, int bw, int64_t value) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= bh * bw) return;
  const int r = i / bw, c = i - r * bw;
  const uint32_t m = bm.row[r];
  if (m >> c & 1u) lab[((size_t)z * H + (y0 + r)) * W + (x0 + c)] = value;
}

// distinct non-zero ids: an open-addressing set, each first insert appends the id to ids[]
__global__ void synth_present_kernel(const int64_t* __restrict__ lab, size_t n, uint64_t* keys, uint32_t* cnt, int64_t* __restrict__ ids, uint32_t cap) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const uint64_t id = (uint64_t)lab[p];
    if (id == 0 || (p > 0 && (uint64_t)lab[p - 1] == id)) continue;  // a run's first voxel speaks for the run
    if (id == kNone) {
      atomicOr(&cnt[1], 1u);
      continue;
    }
    uint32_t h = (uint32_t)mix64(id) & (kSetSlots - 1);
    bool done = false;
    for (uint32_t probe = 0; probe < kSetSlots && !done; ++probe) {
      const uint64_t k = __atomic_load_n(&keys[h], __ATOMIC_RELAXED);
      if (k == id) {
        done = true;
      } else if (k == kNone) {
        const unsigned long long old = atomicCAS((unsigned long long*)&keys[h], (unsigned long long)kNone, (unsigned long long)id);
        if (old == kNone) {
          const uint32_t i = atomicAdd(&cnt[0], 1u);
          if (i < cap && i < kSetSlots / 2) ids[i] = (int64_t)id; else atomicOr(&cnt[1], 1u);
          done = true;
        } else if (old == id) {
          done = true;
        } else {
          h = (h + 1) & (kSetSlots - 1);
        }
      } else {
        h = (h + 1) & (kSetSlots - 1);
      }
    }
    if (!done) atomicOr(&cnt[1], 1u);
  }
}

__global__ void synth_split_mask_kernel(const int64_t* __restrict__ lab, size_t n, int64_t id, uint8_t* __restrict__ mask, int32_t* __restrict__ bg) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const bool m = lab[p] == id;
    mask[p] = m ? 1 : 0;
    bg[p] = m ? 0 : 1;
  }
}

// squared distance to the nearest voxel outside the mask (the volume's border is no background); no such voxel: 2^30
__global__ void synth_split_field_kernel(const uint64_t* __restrict__ key, const uint8_t* __restrict__ mask, size_t n, float* __restrict__ f) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x)
    f[p] = !mask[p] ? 0.f : (key[p] == kNone ? 1073741824.f : (float)(uint32_t)(key[p] >> 32));
}

__global__ void synth_split_write_kernel(int64_t* __restrict__ lab, const uint8_t* __restrict__ mask, const int32_t* __restrict__ frag, int H, int W,
                                         Sections zs, int64_t scale) {
  const size_t plane = (size_t)H * W, n = plane * zs.n;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(i / plane);
    const size_t p = (size_t)(k == 0 ? zs.z[0] : zs.z[1]) * plane + (i - k * plane);
    if (mask[p]) lab[p] = (int64_t)frag[p] * scale;
  }
}

// ---- host side ----

int check_shape(bsmi_synth* h, const int64_t shape[3], int* D, int* H, int* W, size_t* n) {
  if (!h || !shape) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  for (int d = 0; d < 3; ++d)
    if (shape[d] < 1) BSMI_FAIL(BSMI_ERR_INVALID, "shape[%d] = %lld: at least 1", d, (long long)shape[d]);
  const size_t v = (size_t)shape[0] * shape[1] * shape[2];
  if (shape[0] > (1 << 20) || shape[1] > (1 << 20) || shape[2] > (1 << 20) || v > h->max_vox)
    BSMI_FAIL(BSMI_ERR_INVALID, "shape (%lld, %lld, %lld) exceeds the workspace's %zu voxels", (long long)shape[0], (long long)shape[1],
              (long long)shape[2], h->max_vox);
  *D = (int)shape[0];
  *H = (int)shape[1];
  *W = (int)shape[2];
  *n = v;
  return BSMI_OK;
}

int read_num(bsmi_synth* h, uint64_t* num_host, hipStream_t s) {
  if (!num_host) return BSMI_OK;
  BSMI_HIP(hipMemcpyAsync(num_host, h->num_dev, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  BSMI_HIP(hipStreamSynchronize(s));
  return BSMI_OK;
}

void label_i32(bsmi_synth* h, const int32_t* in, int D, int H, int W, int32_t* out, hipStream_t s) {
  const size_t n = (size_t)D * H * W;
  hipLaunchKernelGGL(synth_cc_init_kernel, dim3(grid_for(n)), dim3(256), 0, s, in, n, h->frag);
  hipLaunchKernelGGL(synth_cc_union_kernel, dim3(grid_for(n)), dim3(256), 0, s, in, D, H, W, h->frag);
  cc_rank_roots(n, h->frag, h->num_dev, s);
  hipLaunchKernelGGL(synth_cc_write_kernel, dim3(grid_for(n)), dim3(256), 0, s, n, h->frag, out);
}

// keys of the nearest non-zero voxel of `lab` into h->key_a (offsets along z up to maxd)
void feature_keys(bsmi_synth* h, const int32_t* lab, int D, int H, int W, int maxd, hipStream_t s) {
  const size_t n = (size_t)D * H * W;
  hipLaunchKernelGGL(synth_ft_x_kernel, dim3(grid_for(n)), dim3(256), 0, s, lab, n, W, h->key_a);
  hipLaunchKernelGGL(synth_ft_axis_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const uint64_t*)h->key_a, n, H, (size_t)W, H, h->key_b);
  hipLaunchKernelGGL(synth_ft_axis_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const uint64_t*)h->key_b, n, D, (size_t)H * W, maxd, h->key_a);
}

void argmax_pos(bsmi_synth* h, const float* f, int D, int H, int W, int window, int32_t* pos, hipStream_t s) {
  const size_t n = (size_t)D * H * W;
  const int lo = -(window / 2), hi = window - 1 - window / 2;
  hipLaunchKernelGGL(synth_argmax_x_kernel, dim3(grid_for(n)), dim3(256), 0, s, f, n, W, lo, hi, h->key_a);
  hipLaunchKernelGGL(synth_argmax_axis_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const uint64_t*)h->key_a, n, H, (size_t)W, lo, hi, h->key_b);
  hipLaunchKernelGGL(synth_argmax_axis_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const uint64_t*)h->key_b, n, D, (size_t)H * W, lo, hi, h->key_a);
  hipLaunchKernelGGL(synth_key_pos_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const uint64_t*)h->key_a, n, pos);
}

// out may be `pos` itself: the last kernel no longer reads it
void basins(bsmi_synth* h, const float* f, const int32_t* pos, const uint8_t* mask, int D, int H, int W, int32_t* out, hipStream_t s) {
  const size_t n = (size_t)D * H * W;
  hipLaunchKernelGGL(synth_parent_kernel, dim3(grid_for(n)), dim3(256), 0, s, f, pos, mask, D, H, W, h->frag);
  hipLaunchKernelGGL(synth_root_kernel, dim3(grid_for(n)), dim3(256), 0, s, n, h->frag, h->lab_b);
  cc_rank_roots(n, h->frag, h->num_dev, s);
  hipLaunchKernelGGL(synth_root_write_kernel, dim3(grid_for(n)), dim3(256), 0, s, n, h->frag, (const int32_t*)h->lab_b, out);
}

int check_sections(const int32_t* zs, int nz, int D, Sections* out) {
  if (!zs || nz < 1 || nz > 2) BSMI_FAIL(BSMI_ERR_INVALID, "%d sections: 1 or 2", nz);
  for (int i = 0; i < nz; ++i)
    if (zs[i] < 0 || zs[i] >= D) BSMI_FAIL(BSMI_ERR_INVALID, "section %d outside [0, %d)", zs[i], D);
  out->z[0] = zs[0];
  out->z[1] = nz > 1 ? zs[1] : zs[0];
  out->n = nz;
  return BSMI_OK;
}

}  // namespace
}  // namespace bsmi

using namespace bsmi;

extern "C" {

int bsmi_synth_create(int device, const int64_t max_shape[3], bsmi_synth** out) {
  if (!max_shape || !out) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  for (int d = 0; d < 3; ++d)
    if (max_shape[d] < 1 || max_shape[d] > (1 << 20)) BSMI_FAIL(BSMI_ERR_INVALID, "max_shape[%d] out of range", d);
  const size_t n = (size_t)max_shape[0] * max_shape[1] * max_shape[2];
  if (n >= (1ull << 31)) BSMI_FAIL(BSMI_ERR_INVALID, "%zu voxels: the workspace indexes fewer than 2^31", n);
  BSMI_HIP(hipSetDevice(device));
  bsmi_synth* h = new bsmi_synth();
  h->device = device;
  h->max_vox = n;
  for (int d = 0; d < 3; ++d) h->max_shape[d] = max_shape[d];
  auto alloc = [&](size_t bytes, void** p) -> hipError_t {
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) h->allocs.push_back(*p);
    return e;
  };
  hipError_t e = hipSuccess;
  auto want = [&](size_t bytes, void** p) {
    if (e == hipSuccess) e = alloc(bytes, p);
  };
  want(n * sizeof(int32_t), (void**)&h->frag.par);
  want(n * sizeof(int32_t), (void**)&h->frag.rank);
  want((n / 1024 + 2) * sizeof(uint32_t), (void**)&h->frag.blk);
  want(n * sizeof(uint64_t), (void**)&h->key_a);
  want(n * sizeof(uint64_t), (void**)&h->key_b);
  want(n * sizeof(int32_t), (void**)&h->lab_a);
  want(n * sizeof(int32_t), (void**)&h->lab_b);
  want(n * sizeof(float), (void**)&h->field);
  want(n, (void**)&h->mask);
  want(sizeof(uint64_t), (void**)&h->num_dev);
  want(kParamWords * sizeof(uint32_t), (void**)&h->params);
  want((size_t)kSetSlots * sizeof(uint64_t), (void**)&h->set_keys);
  want(2 * sizeof(uint32_t), (void**)&h->set_cnt);
  if (e != hipSuccess) {
    for (void* p : h->allocs) (void)hipFree(p);
    delete h;
    BSMI_FAIL(BSMI_ERR_HIP, "synth workspace allocation failed: %s", hipGetErrorString(e));
  }
  *out = h;
  return BSMI_OK;
}

int bsmi_synth_destroy(bsmi_synth* h) {
  if (!h) return BSMI_OK;
  (void)hipSetDevice(h->device);
  for (void* p : h->allocs) (void)hipFree(p);
  delete h;
  return BSMI_OK;
}

int bsmi_synth_dilate_points(bsmi_synth* h, const int64_t shape[3], const int32_t* points, int n_points, const uint32_t* bitmaps,
                             const int32_t* bitmap_sizes, const int32_t* iterations, int32_t* out_dev, void* stream) {
  int D, H, W;
  size_t n;
  if (int rc = check_shape(h, shape, &D, &H, &W, &n)) return rc;
  if (!points || !bitmaps || !bitmap_sizes || !iterations || !out_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (n_points < 0 || n_points > kMaxPoints) BSMI_FAIL(BSMI_ERR_INVALID, "%d points: at most %d", n_points, kMaxPoints);
  if (D > kMaxSections) BSMI_FAIL(BSMI_ERR_INVALID, "%d sections: at most %d", D, kMaxSections);
  const size_t lds = (size_t)2 * H * ((W + 31) / 32) * sizeof(uint32_t);
  if (lds > (size_t)kDilateLds)
    BSMI_FAIL(BSMI_ERR_INVALID, "a section of %d x %d needs %zu bytes of LDS for its two bit planes, the kernel has %d", H, W, lds, kDilateLds);
  for (int i = 0; i < n_points; ++i)
    if (points[3 * i] < 0 || points[3 * i] >= D || points[3 * i + 1] < 0 || points[3 * i + 1] >= H || points[3 * i + 2] < 0 || points[3 * i + 2] >= W)
      BSMI_FAIL(BSMI_ERR_INVALID, "point %d (%d, %d, %d) outside the volume", i, points[3 * i], points[3 * i + 1], points[3 * i + 2]);
  for (int z = 0; z < D; ++z) {
    if (bitmap_sizes[2 * z] < 1 || bitmap_sizes[2 * z] > 32 || bitmap_sizes[2 * z + 1] < 1 || bitmap_sizes[2 * z + 1] > 32)
      BSMI_FAIL(BSMI_ERR_INVALID, "section %d: bitmap of %d x %d, at most 32 x 32", z, bitmap_sizes[2 * z], bitmap_sizes[2 * z + 1]);
    if (iterations[z] < 0 || iterations[z] > 10) BSMI_FAIL(BSMI_ERR_INVALID, "section %d: %d iterations, 0..10", z, iterations[z]);
  }
  BSMI_HIP(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  // params: bitmaps [D][32], sizes [D][2], iterations [D], points [n][3]
  uint32_t* bm = h->params;
  int32_t* sz = (int32_t*)(bm + (size_t)32 * D);
  int32_t* it = sz + 2 * D;
  int32_t* pt = it + D;
  BSMI_HIP(hipMemcpyAsync(bm, bitmaps, (size_t)32 * D * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  BSMI_HIP(hipMemcpyAsync(sz, bitmap_sizes, (size_t)2 * D * sizeof(int32_t), hipMemcpyHostToDevice, s));
  BSMI_HIP(hipMemcpyAsync(it, iterations, (size_t)D * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (n_points) BSMI_HIP(hipMemcpyAsync(pt, points, (size_t)3 * n_points * sizeof(int32_t), hipMemcpyHostToDevice, s));
  static DeviceOnce once;
  if (int rc = once.run([&]() -> int {
        BSMI_HIP(hipFuncSetAttribute((const void*)synth_dilate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kDilateLds));
        return BSMI_OK;
      }))
    return rc;
  hipLaunchKernelGGL(synth_dilate_kernel, dim3(D), dim3(256), lds, s, (const int32_t*)pt, n_points, (const uint32_t*)bm, (const int32_t*)sz,
                     (const int32_t*)it, H, W, out_dev);
  BSMI_HIP(hipGetLastError());
  BSMI_HIP(hipStreamSynchronize(s));  // the tables are the caller's host arrays
  return BSMI_OK;
}

int bsmi_synth_label_i32(bsmi_synth* h, const int32_t* in_dev, const int64_t shape[3], int32_t* out_dev, uint64_t* num_host, void* stream) {
  int D, H, W;
  size_t n;
  if (int rc = check_shape(h, shape, &D, &H, &W, &n)) return rc;
  if (!in_dev || !out_dev || in_dev == out_dev) BSMI_FAIL(BSMI_ERR_INVALID, "in and out must be two buffers");
  BSMI_HIP(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  label_i32(h, in_dev, D, H, W, out_dev, s);
  BSMI_HIP(hipGetLastError());
  return read_num(h, num_host, s);
}

int bsmi_synth_expand_i32(bsmi_synth* h, const int32_t* labels_dev, const int64_t shape[3], int depth, int32_t fill, int32_t* out_dev, void* stream) {
  int D, H, W;
  size_t n;
  if (int rc = check_shape(h, shape, &D, &H, &W, &n)) return rc;
  if (!labels_dev || !out_dev || labels_dev == out_dev) BSMI_FAIL(BSMI_ERR_INVALID, "labels and out must be two buffers");
  if (depth < 0 || depth > (1 << 15)) BSMI_FAIL(BSMI_ERR_INVALID, "depth %d out of range", depth);
  BSMI_HIP(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  feature_keys(h, labels_dev, D, H, W, depth, s);
  hipLaunchKernelGGL(synth_expand_write_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const uint64_t*)h->key_a, labels_dev, n,
                     (uint64_t)depth * (uint64_t)depth, fill, out_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_synth_tubes_i32(bsmi_synth* h, const int32_t* fg_dev, const int64_t shape[3], int32_t* out_dev, uint64_t* num_host, void* stream) {
  int D, H, W;
  size_t n;
  if (int rc = check_shape(h, shape, &D, &H, &W, &n)) return rc;
  if (!fg_dev || !out_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  BSMI_HIP(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  uint64_t first = 0;
  label_i32(h, fg_dev, D, H, W, h->lab_a, s);
  BSMI_HIP(hipGetLastError());
  if (int rc = read_num(h, &first, s)) return rc;
  feature_keys(h, h->lab_a, D, H, W, D, s);
  hipLaunchKernelGGL(synth_expand_write_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const uint64_t*)h->key_a, (const int32_t*)h->lab_a, n,
                     (uint64_t)D * (uint64_t)D, (int32_t)(first + 1), h->lab_b);
  label_i32(h, h->lab_b, D, H, W, out_dev, s);
  BSMI_HIP(hipGetLastError());
  return read_num(h, num_host, s);
}

int bsmi_synth_gaussian_f32(bsmi_synth* h, const float* in_dev, const int64_t shape[3], const float* weights, int radius, float* out_dev,
                            void* stream) {
  int D, H, W;
  size_t n;
  if (int rc = check_shape(h, shape, &D, &H, &W, &n)) return rc;
  if (!in_dev || !weights || !out_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (radius < 0 || radius > kMaxRadius) BSMI_FAIL(BSMI_ERR_INVALID, "radius %d: 0..%d", radius, kMaxRadius);
  BSMI_HIP(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  float* w = (float*)h->params;
  BSMI_HIP(hipMemcpyAsync(w, weights, (size_t)(2 * radius + 1) * sizeof(float), hipMemcpyHostToDevice, s));
  float* t0 = (float*)h->key_a;
  float* t1 = (float*)h->key_b;
  hipLaunchKernelGGL(synth_gauss_axis_kernel, dim3(grid_for(n)), dim3(256), 0, s, in_dev, n, D, (size_t)H * W, (const float*)w, radius, t0);
  hipLaunchKernelGGL(synth_gauss_axis_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const float*)t0, n, H, (size_t)W, (const float*)w, radius, t1);
  hipLaunchKernelGGL(synth_gauss_axis_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const float*)t1, n, W, (size_t)1, (const float*)w, radius, out_dev);
  BSMI_HIP(hipGetLastError());
  BSMI_HIP(hipStreamSynchronize(s));  // the weights are the caller's host array
  return BSMI_OK;
}

int bsmi_synth_argmax_filter_f32(bsmi_synth* h, const float* field_dev, const int64_t shape[3], int window, int32_t* pos_dev, void* stream) {
  int D, H, W;
  size_t n;
  if (int rc = check_shape(h, shape, &D, &H, &W, &n)) return rc;
  if (!field_dev || !pos_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (window < 1 || window > 255) BSMI_FAIL(BSMI_ERR_INVALID, "window %d: 1..255", window);
  BSMI_HIP(hipSetDevice(h->device));
  argmax_pos(h, field_dev, D, H, W, window, pos_dev, (hipStream_t)stream);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_synth_basins_f32(bsmi_synth* h, const float* field_dev, const int32_t* pos_dev, const uint8_t* mask_dev, const int64_t shape[3],
                          int32_t* out_dev, uint64_t* num_host, void* stream) {
  int D, H, W;
  size_t n;
  if (int rc = check_shape(h, shape, &D, &H, &W, &n)) return rc;
  if (!field_dev || !pos_dev || !out_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  BSMI_HIP(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  basins(h, field_dev, pos_dev, mask_dev, D, H, W, out_dev, s);
  BSMI_HIP(hipGetLastError());
  return read_num(h, num_host, s);
}

int bsmi_synth_finish_i32(bsmi_synth* h, const int32_t* in_dev, const int64_t shape[3], int drop3, int drop5, int anisotropy, int64_t* out_dev,
                          void* stream) {
  int D, H, W;
  size_t n;
  if (int rc = check_shape(h, shape, &D, &H, &W, &n)) return rc;
  if (!in_dev || !out_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (anisotropy < 1) BSMI_FAIL(BSMI_ERR_INVALID, "anisotropy %d: at least 1", anisotropy);
  const int dout = anisotropy <= D ? (D + anisotropy - 1) / anisotropy : 1;
  BSMI_HIP(hipSetDevice(h->device));
  hipLaunchKernelGGL(synth_finish_kernel, dim3(grid_for((size_t)dout * H * W)), dim3(256), 0, (hipStream_t)stream, in_dev, H, W, anisotropy, dout,
                     drop3 ? 1 : 0, drop5 ? 1 : 0, out_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_synth_grow_boundary_i64(int device, const int64_t* in_dev, const int64_t shape[3], uint64_t seed, int max_steps, int64_t* out_dev,
                                 void* stream) {
  if (!in_dev || !shape || !out_dev || in_dev == out_dev) BSMI_FAIL(BSMI_ERR_INVALID, "in and out must be two buffers");
  if (max_steps < 0 || max_steps > 64) BSMI_FAIL(BSMI_ERR_INVALID, "max_steps %d: 0..64", max_steps);
  for (int d = 0; d < 3; ++d)
    if (shape[d] < 1 || shape[d] > (1 << 20)) BSMI_FAIL(BSMI_ERR_INVALID, "shape out of range on axis %d", d);
  const size_t n = (size_t)shape[0] * shape[1] * shape[2];
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(synth_grow_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, in_dev, (int)shape[0], (int)shape[1], (int)shape[2], seed,
                     max_steps, out_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_synth_merge_i64(int device, int64_t* labels_dev, const int64_t shape[3], const int32_t* sections, int n_sections, int64_t a, int64_t b,
                         void* stream) {
  if (!labels_dev || !shape) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  for (int d = 0; d < 3; ++d)
    if (shape[d] < 1 || shape[d] > (1 << 20)) BSMI_FAIL(BSMI_ERR_INVALID, "shape out of range on axis %d", d);
  Sections zs;
  if (int rc = check_sections(sections, n_sections, (int)shape[0], &zs)) return rc;
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(synth_merge_kernel, dim3(grid_for((size_t)shape[1] * shape[2] * zs.n)), dim3(256), 0, (hipStream_t)stream, labels_dev,
                     (int)shape[1], (int)shape[2], zs, a, b);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_synth_stamp_i64(int device, int64_t* labels_dev, const int64_t shape[3], int z, int y, int x, const uint32_t* bitmap, int bitmap_h,
                         int bitmap_w, int64_t value, void* stream) {
  if (!labels_dev || !shape || !bitmap) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (bitmap_h < 1 || bitmap_h > 32 || bitmap_w < 1 || bitmap_w > 32) BSMI_FAIL(BSMI_ERR_INVALID, "bitmap of %d x %d: at most 32 x 32", bitmap_h, bitmap_w);
  for (int d = 0; d < 3; ++d)
    if (shape[d] < 1 || shape[d] > (1 << 20)) BSMI_FAIL(BSMI_ERR_INVALID, "shape out of range on axis %d", d);
  if (z < 0 || z >= shape[0] || y < 0 || y + bitmap_h > shape[1] || x < 0 || x + bitmap_w > shape[2])
    BSMI_FAIL(BSMI_ERR_INVALID, "stamp of %d x %d at (%d, %d, %d) leaves the volume", bitmap_h, bitmap_w, z, y, x);
  Bitmap bm{};
  for (int r = 0; r < bitmap_h; ++r) bm.row[r] = bitmap[r];
  BSMI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(synth_stamp_kernel, dim3(4), dim3(256), 0, (hipStream_t)stream, labels_dev, (int)shape[1], (int)shape[2], z, y, x, bm, bitmap_h,
                     bitmap_w, value);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_synth_present_i64(bsmi_synth* h, const int64_t* labels_dev, uint64_t n_voxels, int64_t* ids_dev, uint32_t capacity, uint32_t* count_host,
                           void* stream) {
  if (!h || !labels_dev || !ids_dev || !count_host) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (n_voxels >= (1ull << 40)) BSMI_FAIL(BSMI_ERR_INVALID, "too many voxels");
  BSMI_HIP(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  BSMI_HIP(hipMemsetAsync(h->set_keys, 0xff, (size_t)kSetSlots * sizeof(uint64_t), s));
  BSMI_HIP(hipMemsetAsync(h->set_cnt, 0, 2 * sizeof(uint32_t), s));
  if (n_voxels)
    hipLaunchKernelGGL(synth_present_kernel, dim3(grid_for((size_t)n_voxels)), dim3(256), 0, s, labels_dev, (size_t)n_voxels, h->set_keys, h->set_cnt,
                       ids_dev, capacity);
  BSMI_HIP(hipGetLastError());
  uint32_t cnt[2];
  BSMI_HIP(hipMemcpyAsync(cnt, h->set_cnt, sizeof cnt, hipMemcpyDeviceToHost, s));
  BSMI_HIP(hipStreamSynchronize(s));
  if (cnt[1]) BSMI_FAIL(BSMI_ERR_OVERFLOW, "more distinct labels (%u) than the presence table (%u) or the ids buffer (%u) holds", cnt[0], kSetSlots / 2, capacity);
  *count_host = cnt[0];
  return BSMI_OK;
}

int bsmi_synth_split_i64(bsmi_synth* h, int64_t* labels_dev, const int64_t shape[3], int64_t id, int window, const int32_t* sections, int n_sections,
                         int64_t scale, uint64_t* num_host, void* stream) {
  int D, H, W;
  size_t n;
  if (int rc = check_shape(h, shape, &D, &H, &W, &n)) return rc;
  if (!labels_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (window < 1 || window > 255) BSMI_FAIL(BSMI_ERR_INVALID, "window %d: 1..255", window);
  Sections zs;
  if (int rc = check_sections(sections, n_sections, D, &zs)) return rc;
  BSMI_HIP(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(synth_split_mask_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const int64_t*)labels_dev, n, id, h->mask, h->lab_a);
  feature_keys(h, h->lab_a, D, H, W, D, s);
  hipLaunchKernelGGL(synth_split_field_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const uint64_t*)h->key_a, (const uint8_t*)h->mask, n, h->field);
  argmax_pos(h, h->field, D, H, W, window, h->lab_a, s);
  basins(h, h->field, h->lab_a, h->mask, D, H, W, h->lab_a, s);
  hipLaunchKernelGGL(synth_split_write_kernel, dim3(grid_for((size_t)H * W * zs.n)), dim3(256), 0, s, labels_dev, (const uint8_t*)h->mask,
                     (const int32_t*)h->lab_a, H, W, zs, scale);
  BSMI_HIP(hipGetLastError());
  return read_num(h, num_host, s);
}

}  // extern "C"

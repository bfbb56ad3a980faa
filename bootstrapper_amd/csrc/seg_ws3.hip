// Watershed fragments, 3-D mode (fragments_in_xy = False): the parallel steps as plain kernels, then ONE sequential flood --
// a single wave on the device, or the host's (flood_host.cpp) when the handle says so (bsmi_seg_set_host_flood).
#include "seg_internal.h"

#include "dev_guard.h"  // last: routes hipMalloc / hipFree through the guarded allocator (BSMI_GUARD_MB)

namespace bsmi {

void host_flood3(int D, int H, int W, const uint8_t* mask, const int32_t* d2, int32_t* lab);  // flood_host.cpp

// ------------------------------------------------------------------------------------------
// fragments_in_xy = False (reference post/ws.py:97-110): one 3-D domain.  Same steps as the per-slice path --
// mask (a_z + a_y + a_x >= 383), exact squared EDT, separable reflect max filter, 6-connected maxima components in
// raster order, literal replay of skimage's heap -- but the flood is ONE sequential queue over the whole volume (the
// reference's own algorithm), so this mode is latency-bound on a single wave; the parallel steps are plain kernels.
// ------------------------------------------------------------------------------------------
constexpr int INF3 = 1 << 28;

__global__ void ws3_mask_kernel(const uint8_t* __restrict__ affs, size_t n, uint8_t* __restrict__ mask, int* __restrict__ any_bg) {
  int bg = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int m = (int)affs[i] + (int)affs[n + i] + (int)affs[2 * n + i] >= 383;
    mask[i] = (uint8_t)m;
    bg |= !m;
  }
  if (bg) atomicOr(any_bg, 1);
}

// x pass: squared distance to the nearest background voxel of the same row (INF3 if none); one thread per row
__global__ void ws3_edt_x_kernel(const uint8_t* __restrict__ mask, int rows, int W, int32_t* __restrict__ g) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += gridDim.x * blockDim.x) {
    const uint8_t* m = mask + (size_t)r * W;
    int32_t* o = g + (size_t)r * W;
    int last = -INF3;
    for (int x = 0; x < W; ++x) {
      if (!m[x]) last = x;
      o[x] = last <= -INF3 ? INF3 : (x - last) * (x - last);
    }
    last = INF3;
    for (int x = W - 1; x >= 0; --x) {
      if (!m[x]) last = x;
      if (last < INF3) {
        const int d = (last - x) * (last - x);
        if (d < o[x]) o[x] = d;
      }
    }
  }
}

// out[p] = min over k along `axis` of in[p with coordinate k] + (coord - k)^2 (exact; brute force over the axis)
__global__ void ws3_edt_axis_kernel(const int32_t* __restrict__ in, int D, int H, int W, int axis, int32_t* __restrict__ out) {
  const size_t n = (size_t)D * H * W;
  const size_t stride = axis == 0 ? (size_t)H * W : (size_t)W;
  const int len = axis == 0 ? D : H;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const int c = axis == 0 ? (int)(p / ((size_t)H * W)) : (int)((p / W) % H);
    const size_t base = p - (size_t)c * stride;
    int best = INF3;
    for (int k = 0; k < len; ++k) {
      const int v = in[base + (size_t)k * stride];
      if (v >= INF3) continue;
      const int d = v + (c - k) * (c - k);
      best = d < best ? d : best;
    }
    out[p] = best;
  }
}

// scipy's result when the volume has no background voxel at all: as if the only one sat at index (-1, 0, 0)
__global__ void ws3_edt_nobg_kernel(int D, int H, int W, const int* __restrict__ any_bg, int32_t* __restrict__ d2) {
  if (*any_bg) return;
  const size_t n = (size_t)D * H * W;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(p % W), y = (int)((p / W) % H), z = (int)(p / ((size_t)H * W));
    d2[p] = (z + 1) * (z + 1) + y * y + x * x;
  }
}

// maximum over the window [c - size/2, c + size - 1 - size/2] along `axis`, border mode reflect (edge duplicated)
__global__ void ws3_maxfilter_kernel(const int32_t* __restrict__ in, int D, int H, int W, int axis, int size, int32_t* __restrict__ out) {
  const size_t n = (size_t)D * H * W;
  const size_t stride = axis == 0 ? (size_t)H * W : (axis == 1 ? (size_t)W : 1);
  const int len = axis == 0 ? D : (axis == 1 ? H : W);
  const int left = size / 2, right = size - 1 - size / 2;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const int c = axis == 0 ? (int)(p / ((size_t)H * W)) : (axis == 1 ? (int)((p / W) % H) : (int)(p % W));
    const size_t base = p - (size_t)c * stride;
    int m = INT32_MIN;
    for (int k = c - left; k <= c + right; ++k) {
      const int v = in[base + (size_t)reflect_dup(k, len) * stride];
      m = v > m ? v : m;
    }
    out[p] = m;
  }
}

// maxima flag (as the uint64 "value" array of the cc kernels) and union-find initialisation
__global__ void ws3_maxima_kernel(const int32_t* __restrict__ d2, const int32_t* __restrict__ mf, size_t n, uint64_t* __restrict__ flag, FragWs w) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const bool mx = d2[p] == mf[p];
    flag[p] = mx ? 1ull : 0ull;
    w.par[p] = mx ? (int32_t)p : -1;
  }
}

// 6-connected union of equal non-zero values with the three raster-preceding neighbours
__global__ void cc6_union_kernel(const uint64_t* __restrict__ x, int D, int H, int W, FragWs w) {
  const size_t n = (size_t)D * H * W, hw = (size_t)H * W;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const uint64_t v = x[p];
    if (!v) continue;
    const int xx = (int)(p % W), y = (int)((p / W) % H), z = (int)(p / hw);
    const bool ok[3] = {z > 0, y > 0, xx > 0};
    const size_t st[3] = {hw, (size_t)W, 1};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (!ok[d] || x[p - st[d]] != v) continue;
      cc_unite(w.par, (int)p, (int)(p - st[d]));
    }
  }
}

// markers: component rank of the maxima inside the mask, 0 elsewhere
__global__ void ws3_markers_kernel(const uint64_t* __restrict__ flag, const uint8_t* __restrict__ mask, size_t n, FragWs w, int32_t* __restrict__ lab,
                                   uint64_t* __restrict__ seeds) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const int l = flag[p] ? (int)w.rank[cc_find(w.par, (int)p)] : 0;
    lab[p] = mask[p] ? l : 0;
    if (seeds) seeds[p] = (uint64_t)l;
  }
}

// heap entry of the 3-D flood: [63:46] = MAXD2 - d2 (18 bit) | [45:23] = age (23 bit) | [22:0] = voxel index
__device__ __forceinline__ bool flood3_smaller(uint64_t a, uint64_t b) { return (a >> 23) < (b >> 23); }

__global__ __launch_bounds__(64) void ws3_flood_kernel(int D, int H, int W, WsScratch s, uint64_t* __restrict__ hg, uint64_t* __restrict__ frags) {
  __shared__ uint64_t hl[8192];
  constexpr int LH = 8192;
  const size_t n = (size_t)D * H * W, hw = (size_t)H * W;
  const int lane = threadIdx.x;
  const uint8_t* mask = s.mask;
  const int32_t* d2 = s.d2;
  int32_t* lab = s.lab;
  // As in ws_flood_kernel the wave walks the one sequential loop in lockstep: lane 0 writes the LDS part of the heap, every
  // lane its HBM part (same address, same value: each lane's later loads then follow its own stores), lanes k < 6 fetch
  // neighbour k of the popped voxel in one round of loads issued before the sift-down, and write the labels.
  {
    constexpr uint64_t MAXD2 = (1u << 18) - 1;
    size_t items = 0;
    auto hget = [&](size_t i) -> uint64_t { return i < LH ? hl[i] : hg[i - LH]; };
    auto hset = [&](size_t i, uint64_t v) {
      if (i < LH) {
        if (lane == 0) hl[i] = v;
      } else {
        hg[i - LH] = v;
      }
    };
    auto push = [&](uint64_t it) {
      size_t c = items++;
      while (c > 0) {
        const size_t p = (c + 1) / 2 - 1;
        const uint64_t pv = hget(p);
        if (flood3_smaller(it, pv)) { hset(c, pv); c = p; } else break;
      }
      hset(c, it);
    };
    for (size_t i0 = 0; i0 < n; i0 += 64) {
      const size_t i = i0 + lane;
      const int li = i < n ? lab[i] : 0;
      unsigned long long seeds = __ballot(li != 0);
      while (seeds) {
        const int k = __ffsll(seeds) - 1;
        seeds &= seeds - 1;
        const size_t j = i0 + k;
        push(((MAXD2 - (uint64_t)d2[j]) << 46) | (uint64_t)j);
      }
    }
    uint64_t age = 0;
    const int k8 = lane & 7;
    const long long dq = k8 == 0 ? -(long long)hw : (k8 == 1 ? -(long long)W : (k8 == 2 ? -1 : (k8 == 3 ? 1 : (k8 == 4 ? (long long)W : (long long)hw))));
    while (items > 0) {
      const uint64_t e = hget(0);
      --items;
      const size_t idx = (size_t)(e & 0x7fffffu);
      const int x = (int)(idx % W), y = (int)((idx / W) % H), z = (int)(idx / hw);
      // neighbour order [-HW, -W, -1, +1, +W, +HW]
      const bool okk = k8 == 0 ? z > 0 : (k8 == 1 ? y > 0 : (k8 == 2 ? x > 0 : (k8 == 3 ? x < W - 1 : (k8 == 4 ? y < H - 1 : z < D - 1))));
      const size_t qk = okk ? (size_t)((long long)idx + dq) : idx;
      int lme = 0, mk = 0, lk = 0, dk = 0;
      if (lane < 6) {
        lme = lab[idx];
        mk = mask[qk];
        lk = lab[qk];
        dk = d2[qk];
      }
      const int l = __builtin_amdgcn_readfirstlane(lme);
      if (items > 0) {
        const uint64_t last = hget(items);
        size_t i = 0;
        for (;;) {
          const size_t c1 = 2 * i + 1, c2 = c1 + 1;
          if (c1 >= items) break;
          const uint64_t v1 = hget(c1);
          size_t sm = i;
          uint64_t smv = last;
          if (flood3_smaller(v1, smv)) { sm = c1; smv = v1; }
          if (c2 < items) {
            const uint64_t v2 = hget(c2);
            if (flood3_smaller(v2, smv)) { sm = c2; smv = v2; }
          }
          if (sm == i) break;
          hset(i, smv);
          i = sm;
        }
        hset(i, last);
      }
      const int cand = (lane < 6 && okk && mk && lk == 0) ? 1 : 0;
      const int qlo = (int)qk;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        if (!__shfl(cand, k)) continue;  // wave uniform
        const size_t q = (size_t)(uint32_t)__shfl(qlo, k);
        const uint64_t dd = (uint64_t)(uint32_t)__shfl(dk, k);
        ++age;
        if (lane < 6) lab[q] = l;
        push(((MAXD2 - dd) << 46) | (age << 23) | (uint64_t)q);
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  for (size_t i = lane; i < n; i += 64) {
    const int l = lab[i];
    frags[i] = l ? (uint64_t)l : 0ull;
  }
}

// fragments of the 3-D mode = the flooded labels (bsmi_seg_set_host_flood: the flood ran on the host)
__global__ void ws3_labels_out_kernel(const int32_t* __restrict__ lab, size_t n, uint64_t* __restrict__ frags) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) frags[i] = (uint64_t)(uint32_t)lab[i];
}

int fragments_3d(bsmi_seg* h, const uint8_t* affs_dev, int D, int H, int W, int min_seed_distance, uint64_t* frags_dev,
                 uint64_t* max_id_dev, uint64_t* seeds_dev, hipStream_t s) {
  const size_t n = (size_t)D * H * W;
  // the device flood's packed queue entry (ws3_flood_kernel); the host flood widens its entry where needed (flood_host.cpp)
  if (!h->host_flood3 && (n >= ((size_t)1 << 23) || (size_t)D * D + (size_t)H * H + (size_t)W * W + 2 * D + 1 >= ((size_t)1 << 18)))
    BSMI_FAIL(BSMI_ERR_INVALID, "3-D watershed: volumes of 2^23 voxels or more are not supported by the flood's queue entries");
  WsScratch& w = h->ws;
  FragWs& f = h->frag;
  const int bs = 256;
  const int grid = (int)std::min<size_t>((n + bs - 1) / bs, 4096);
  int* any_bg = (int*)h->status_dev;
  BSMI_HIP(hipMemsetAsync(any_bg, 0, sizeof(int), s));
  hipLaunchKernelGGL(ws3_mask_kernel, dim3(grid), dim3(bs), 0, s, affs_dev, n, w.mask, any_bg);
  hipLaunchKernelGGL(ws3_edt_x_kernel, dim3((D * H + 63) / 64), dim3(64), 0, s, (const uint8_t*)w.mask, D * H, W, w.g);
  hipLaunchKernelGGL(ws3_edt_axis_kernel, dim3(grid), dim3(bs), 0, s, (const int32_t*)w.g, D, H, W, 1, w.mf);
  hipLaunchKernelGGL(ws3_edt_axis_kernel, dim3(grid), dim3(bs), 0, s, (const int32_t*)w.mf, D, H, W, 0, w.d2);
  hipLaunchKernelGGL(ws3_edt_nobg_kernel, dim3(grid), dim3(bs), 0, s, D, H, W, (const int*)any_bg, w.d2);
  hipLaunchKernelGGL(ws3_maxfilter_kernel, dim3(grid), dim3(bs), 0, s, (const int32_t*)w.d2, D, H, W, 2, min_seed_distance, w.g);
  hipLaunchKernelGGL(ws3_maxfilter_kernel, dim3(grid), dim3(bs), 0, s, (const int32_t*)w.g, D, H, W, 1, min_seed_distance, w.mf);
  hipLaunchKernelGGL(ws3_maxfilter_kernel, dim3(grid), dim3(bs), 0, s, (const int32_t*)w.mf, D, H, W, 0, min_seed_distance, w.g);
  f.par = w.par;
  hipLaunchKernelGGL(ws3_maxima_kernel, dim3(grid), dim3(bs), 0, s, (const int32_t*)w.d2, (const int32_t*)w.g, n, h->crop_tmp, f);
  hipLaunchKernelGGL(cc6_union_kernel, dim3(grid), dim3(bs), 0, s, (const uint64_t*)h->crop_tmp, D, H, W, f);
  cc_rank_roots(n, f, max_id_dev, s);
  hipLaunchKernelGGL(ws3_markers_kernel, dim3(grid), dim3(bs), 0, s, (const uint64_t*)h->crop_tmp, (const uint8_t*)w.mask, n, f, w.lab, seeds_dev);
  if (h->host_flood3) {
    // the caller waits for this one result: mask, distances and markers to the host, the sequential flood there, labels back
    BSMI_HIP(hipGetLastError());
    std::vector<uint8_t> hmask(n);
    std::vector<int32_t> hd2(n), hlab(n);
    BSMI_HIP(hipMemcpyAsync(hmask.data(), w.mask, n, hipMemcpyDeviceToHost, s));
    BSMI_HIP(hipMemcpyAsync(hd2.data(), w.d2, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    BSMI_HIP(hipMemcpyAsync(hlab.data(), w.lab, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    BSMI_HIP(hipStreamSynchronize(s));
    host_flood3(D, H, W, hmask.data(), hd2.data(), hlab.data());
    BSMI_HIP(hipMemcpyAsync(w.lab, hlab.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(ws3_labels_out_kernel, dim3(grid), dim3(bs), 0, s, (const int32_t*)w.lab, n, frags_dev);
    BSMI_HIP(hipGetLastError());
    BSMI_HIP(hipStreamSynchronize(s));  // (the host buffers go out of scope)
    return BSMI_OK;
  }
  hipLaunchKernelGGL(ws3_flood_kernel, dim3(1), dim3(64), 0, s, D, H, W, w, h->flood_spill, frags_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}
}  // namespace bsmi

// Label volumes on the device: LUT relabel, the blockwise fragment clean-up, the connected-components family (26-connected
// relabel, thresholded affinities; the ranking of union-find roots, which the 3-D fragments mode shares), label statistics
// and the label table of `bs refine`.
#include "seg_internal.h"

#include "dev_guard.h"  // last: routes hipMalloc / hipFree through the guarded allocator (BSMI_GUARD_MB)

namespace bsmi {

// segmentation lookup: out[p] = vals[k] where keys[k] == in[p] (keys ascending), 0 stays 0, an id
// that is not a key maps to itself.  volara Relabel + LUT (post/watershed.py:187-202).
__global__ void lut_relabel_kernel(const uint64_t* __restrict__ in, size_t n, const uint64_t* __restrict__ keys,
                                   const uint64_t* __restrict__ vals, uint64_t m, uint64_t* __restrict__ out) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const uint64_t f = in[p];
    uint64_t r = f;
    if (f && m) {
      uint64_t lo = 0, hi = m;
      while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (keys[mid] < f) lo = mid + 1; else hi = mid;
      }
      if (lo < m && keys[lo] == f) r = vals[lo];
    }
    out[p] = r;
  }
}

// The same for T value columns at once (one segmentation per threshold out of one fragment volume): a thread takes RUN
// consecutive voxels and searches only when the id changes -- fragments are compact, the next voxel along x mostly carries
// the same id --, and the one look-up serves all T outputs (three single passes over the slab: 17 dependent L2 reads per
// voxel and pass, 0.75 ms per pass and 20 blocks; this: one pass).
constexpr int kLutMaxColumns = 8;
struct LutColumns {
  const uint64_t* vals[kLutMaxColumns];
  uint64_t* out[kLutMaxColumns];
};
__global__ void lut_relabel_multi_kernel(const uint64_t* __restrict__ in, size_t n, const uint64_t* __restrict__ keys, uint64_t m, int T,
                                         LutColumns c) {
  constexpr int RUN = 8;
  const size_t nruns = (n + RUN - 1) / RUN;
  for (size_t r0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r0 < nruns; r0 += (size_t)gridDim.x * blockDim.x) {
    uint64_t last = 0, idx = m;  // idx == m: no key
    const size_t p0 = r0 * RUN, p1 = p0 + RUN < n ? p0 + RUN : n;
    for (size_t p = p0; p < p1; ++p) {
      const uint64_t f = in[p];
      if (f != last) {
        last = f;
        idx = m;
        if (f && m) {
          uint64_t lo = 0, hi = m;
          while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (keys[mid] < f) lo = mid + 1; else hi = mid;
          }
          if (lo < m && keys[lo] == f) idx = lo;
        }
      }
      for (int t = 0; t < T; ++t) c.out[t][p] = idx < m ? c.vals[t][idx] : f;
    }
  }
}

// ------------------------------------------------------------------------------------------
// blockwise fragment post-processing (reference post/blockwise/watershed_frags.py:148-156,181-224)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void frag_stats_body(const uint8_t* __restrict__ affs, const uint64_t* __restrict__ frags, size_t n, const FragWs& w) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const uint64_t f = frags[p];
    if (!f) continue;
    if (f >= w.id_cap) { atomicOr(w.flags, 1u); continue; }
    atomicAdd(&w.lsum[f], (unsigned long long)((uint32_t)affs[p] + affs[n + p] + affs[2 * n + p]));
    atomicAdd(&w.lcnt[f], 1u);
  }
}
__global__ void frag_stats_kernel(const uint8_t* __restrict__ affs, const uint64_t* __restrict__ frags, size_t n, FragWs w) { frag_stats_body(affs, frags, n, w); }
__global__ void frag_stats_batch_kernel(const BatchBlock* __restrict__ tab, size_t n) {
  const BatchBlock& b = tab[blockIdx.y];
  frag_stats_body(b.f.affs, b.f.frags, n, b.frag);
}

// filter_avg_fragments: mean of the 3-channel average affinity (u8 / 255) below filter_value;
// remove_small_objects: fewer than min_size voxels.  Both decided per fragment on the read ROI
// and recorded in bit 31 of the count.  The reference accumulates float64 values
// ((a0/255 + a1/255) + a2/255) / 3 in raster order (numpy mean over axis 0, scipy.ndimage.mean =
// bincount); the exact rational S / (765 n) decides unless it lies within 1e-9 of the filter,
// where the float64 accumulation is replayed sequentially so that the outcome is the reference's.
__device__ __forceinline__ void frag_decide_body(const uint8_t* __restrict__ affs, const uint64_t* __restrict__ frags, size_t n, const FragWs& w,
                                   double filter_value, long long min_size) {
  for (uint32_t f = blockIdx.x * blockDim.x + threadIdx.x; f < w.id_cap; f += gridDim.x * blockDim.x) {
    const uint32_t c = w.lcnt[f];
    if (!c || !f) continue;
    bool drop = false;
    if (filter_value > 0.0) {
      double mean = (double)w.lsum[f] / (765.0 * (double)c);
      if (fabs(mean - filter_value) <= 1e-9) {
        double sum = 0.0;
        for (size_t p = 0; p < n; ++p)
          if (frags[p] == f)
            sum += (((double)affs[p] / 255.0 + (double)affs[n + p] / 255.0) + (double)affs[2 * n + p] / 255.0) / 3.0;
        mean = sum / (double)c;
      }
      drop = mean < filter_value;
    }
    if (min_size > 0) drop = drop || (long long)c < min_size;
    if (drop) w.lcnt[f] = c | 0x80000000u;
  }
}
__global__ void frag_decide_kernel(const uint8_t* __restrict__ affs, const uint64_t* __restrict__ frags, size_t n, FragWs w,
                                   double filter_value, long long min_size) { frag_decide_body(affs, frags, n, w, filter_value, min_size); }
__global__ void frag_decide_batch_kernel(const BatchBlock* __restrict__ tab, size_t n, double filter_value, long long min_size) {
  const BatchBlock& b = tab[blockIdx.y];
  frag_decide_body(b.f.affs, b.f.frags, n, b.frag, filter_value, min_size);
}

__device__ __forceinline__ void frag_filter_body(uint64_t* __restrict__ frags, size_t n, const FragWs& w) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const uint64_t f = frags[p];
    if (!f || f >= w.id_cap) continue;
    if (w.lcnt[f] & 0x80000000u) frags[p] = 0;
  }
}
__global__ void frag_filter_kernel(uint64_t* __restrict__ frags, size_t n, FragWs w) { frag_filter_body(frags, n, w); }
__global__ void frag_filter_batch_kernel(const BatchBlock* __restrict__ tab, size_t n) {
  const BatchBlock& b = tab[blockIdx.y];
  frag_filter_body(b.f.frags, n, b.frag);
}

__device__ __forceinline__ void crop_u64_body(const uint64_t* __restrict__ in, int H, int W, int oz, int oy, int ox, int cd, int ch,
                                int cw, uint64_t* __restrict__ out) {
  const size_t n = (size_t)cd * ch * cw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % cw);
    const int y = (int)((i / cw) % ch);
    const int z = (int)(i / ((size_t)cw * ch));
    out[i] = in[((size_t)(z + oz) * H + (y + oy)) * W + (x + ox)];
  }
}
__global__ void crop_u64_kernel(const uint64_t* __restrict__ in, int H, int W, int oz, int oy, int ox, int cd, int ch,
                                int cw, uint64_t* __restrict__ out) { crop_u64_body(in, H, W, oz, oy, ox, cd, ch, cw, out); }
__global__ void crop_u64_batch_kernel(const BatchBlock* __restrict__ tab, int H, int W, int oz, int oy, int ox, int cd, int ch, int cw) {
  const BatchBlock& b = tab[blockIdx.y];
  crop_u64_body(b.f.frags, H, W, oz, oy, ox, cd, ch, cw, b.crop_tmp);
}

__device__ __forceinline__ void cc26_init_body(const uint64_t* __restrict__ x, size_t n, const FragWs& w) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x)
    w.par[p] = x[p] ? (int32_t)p : -1;
}
__global__ void cc26_init_kernel(const uint64_t* __restrict__ x, size_t n, FragWs w) { cc26_init_body(x, n, w); }
__global__ void cc26_init_batch_kernel(const BatchBlock* __restrict__ tab, size_t n) {
  const BatchBlock& b = tab[blockIdx.y];
  cc26_init_body(b.crop_tmp, n, b.frag);
}

// unite every voxel with its 13 raster-preceding neighbours of equal value (26-connectivity)
__device__ __forceinline__ void cc26_union_body(const uint64_t* __restrict__ x, int D, int H, int W, const FragWs& w) {
  const size_t n = (size_t)D * H * W;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const uint64_t v = x[p];
    if (!v) continue;
    const int xx = (int)(p % W);
    const int y = (int)((p / W) % H);
    const int z = (int)(p / ((size_t)W * H));
    for (int dz = -1; dz <= 0; ++dz)
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          if (dz == 0 && (dy > 0 || (dy == 0 && dx >= 0))) continue;
          const int zz = z + dz, yy = y + dy, x2 = xx + dx;
          if (zz < 0 || yy < 0 || yy >= H || x2 < 0 || x2 >= W) continue;
          const size_t q = ((size_t)zz * H + yy) * W + x2;
          if (x[q] != v) continue;
          cc_unite(w.par, (int)p, (int)q);
        }
  }
}
__global__ void cc26_union_kernel(const uint64_t* __restrict__ x, int D, int H, int W, FragWs w) { cc26_union_body(x, D, H, W, w); }
__global__ void cc26_union_batch_kernel(const BatchBlock* __restrict__ tab, int D, int H, int W) {
  const BatchBlock& b = tab[blockIdx.y];
  cc26_union_body(b.crop_tmp, D, H, W, b.frag);
}

// roots per 1024-voxel block (raster order), then one workgroup scans the block counts
__device__ __forceinline__ void cc26_count_body(size_t n, const FragWs& w) {
  __shared__ uint32_t cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  const size_t p = (size_t)blockIdx.x * 1024 + threadIdx.x;
  if (p < n && w.par[p] == (int32_t)p) atomicAdd(&cnt, 1u);
  __syncthreads();
  if (threadIdx.x == 0) w.blk[blockIdx.x] = cnt;
}
__global__ __launch_bounds__(1024) void cc26_count_kernel(size_t n, FragWs w) { cc26_count_body(n, w); }
__global__ __launch_bounds__(1024) void cc26_count_batch_kernel(const BatchBlock* __restrict__ tab, size_t n) {
  const BatchBlock& b = tab[blockIdx.y];
  cc26_count_body(n, b.frag);
}

__device__ __forceinline__ void cc26_scan_body(uint32_t nblk, const FragWs& w, uint64_t* num_out) {
  __shared__ uint32_t sh[1024];
  const uint32_t chunk = (nblk + 1023) / 1024;
  const uint32_t c0 = threadIdx.x * chunk, c1 = min(nblk, c0 + chunk);
  uint32_t s = 0;
  for (uint32_t i = c0; i < c1; ++i) s += w.blk[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t acc = 0;
    for (int t = 0; t < 1024; ++t) { const uint32_t c = sh[t]; sh[t] = acc; acc += c; }
    *num_out = acc;
  }
  __syncthreads();
  uint32_t acc = sh[threadIdx.x];
  for (uint32_t i = c0; i < c1; ++i) { const uint32_t c = w.blk[i]; w.blk[i] = acc; acc += c; }
}
__global__ __launch_bounds__(1024) void cc26_scan_kernel(uint32_t nblk, FragWs w, uint64_t* num_out) { cc26_scan_body(nblk, w, num_out); }
__global__ __launch_bounds__(1024) void cc26_scan_batch_kernel(const BatchBlock* __restrict__ tab, uint32_t nblk) {
  const BatchBlock& b = tab[blockIdx.y];
  cc26_scan_body(nblk, b.frag, b.f.num);
}

// rank of every root = number of roots before it in raster order (+1)
__device__ __forceinline__ void cc26_rank_body(size_t n, const FragWs& w) {
  __shared__ uint32_t sh[1024];
  const size_t p = (size_t)blockIdx.x * 1024 + threadIdx.x;
  const uint32_t flag = (p < n && w.par[p] == (int32_t)p) ? 1u : 0u;
  sh[threadIdx.x] = flag;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {  // inclusive Hillis-Steele scan
    const uint32_t v = threadIdx.x >= (unsigned)o ? sh[threadIdx.x - o] : 0u;
    __syncthreads();
    sh[threadIdx.x] += v;
    __syncthreads();
  }
  if (flag) w.rank[p] = (int32_t)(w.blk[blockIdx.x] + sh[threadIdx.x]);
}
__global__ __launch_bounds__(1024) void cc26_rank_kernel(size_t n, FragWs w) { cc26_rank_body(n, w); }
__global__ __launch_bounds__(1024) void cc26_rank_batch_kernel(const BatchBlock* __restrict__ tab, size_t n) {
  const BatchBlock& b = tab[blockIdx.y];
  cc26_rank_body(n, b.frag);
}

void cc_rank_roots(size_t n, const FragWs& f, uint64_t* num_out, hipStream_t s) {
  const uint32_t nblk = (uint32_t)((n + 1023) / 1024);
  hipLaunchKernelGGL(cc26_count_kernel, dim3(nblk), dim3(1024), 0, s, n, f);
  hipLaunchKernelGGL(cc26_scan_kernel, dim3(1), dim3(1024), 0, s, nblk, f, num_out);
  hipLaunchKernelGGL(cc26_rank_kernel, dim3(nblk), dim3(1024), 0, s, n, f);
}

__device__ __forceinline__ void cc26_write_body(const uint64_t* __restrict__ x, size_t n, const FragWs& w, uint64_t id_offset, uint64_t* __restrict__ out) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    if (!x[p]) { out[p] = 0; continue; }
    out[p] = id_offset + (uint64_t)w.rank[cc_find(w.par, (int)p)];
  }
}
__global__ void cc26_write_kernel(const uint64_t* __restrict__ x, size_t n, FragWs w, uint64_t id_offset, uint64_t* __restrict__ out) { cc26_write_body(x, n, w, id_offset, out); }
__global__ void cc26_write_batch_kernel(const BatchBlock* __restrict__ tab, size_t n) {
  const BatchBlock& b = tab[blockIdx.y];
  cc26_write_body(b.crop_tmp, n, b.frag, b.f.id_offset, b.f.labels);
}

// thresholded-affinity connected components (reference post/cc.py:7-74): voxel p is linked with p + e_d when
// affs[d][p] > cut; a voxel is labelled if it has a link of its own (even one that leaves the volume) or is the far end
// of a neighbour's link.  Roots are the raster-first voxels of their components, so the cc26 ranking kernels give the
// reference's numbering (depth-first fills started in raster order).
__global__ void ccaff_init_kernel(size_t n, FragWs w, uint64_t* __restrict__ touched) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    w.par[p] = (int32_t)p;
    touched[p] = 0;
  }
}

__global__ void ccaff_union_kernel(const uint8_t* __restrict__ affs, int D, int H, int W, int cut, FragWs w, uint64_t* __restrict__ touched) {
  const size_t n = (size_t)D * H * W, hw = (size_t)H * W;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(p % W), y = (int)((p / W) % H), z = (int)(p / hw);
    const bool ok[3] = {z + 1 < D, y + 1 < H, x + 1 < W};
    const size_t st[3] = {hw, (size_t)W, 1};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if ((int)affs[(size_t)d * n + p] <= cut) continue;
      touched[p] = 1;
      if (!ok[d]) continue;
      const size_t q = p + st[d];
      touched[q] = 1;
      cc_unite(w.par, (int)p, (int)q);
    }
  }
}

__global__ void ccaff_finalize_kernel(size_t n, FragWs w, const uint64_t* __restrict__ touched) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x)
    if (!touched[p]) w.par[p] = -1;
}

// label table of a block (reference refine.py:98-109 `_global_sizes`, :228-250 z extents): every distinct non-zero id
// with its voxel count and the first / last z slice it occurs in.  Runs of equal ids along x are counted once.
__global__ void ltab_clear_kernel(AggWs w) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < w.icap; i += (size_t)gridDim.x * blockDim.x) {
    w.idkeys[i] = HEMPTY;
    w.tcount[i] = 0;
    w.tzmin[i] = 0x7fffffff;
    w.tzmax[i] = -0x7fffffff;
  }
}

__global__ void ltab_scan_kernel(const uint64_t* __restrict__ lab, int D, int H, int W, int z0, AggWs w) {
  const size_t nrows = (size_t)D * H;
  for (size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x; row < nrows; row += (size_t)gridDim.x * blockDim.x) {
    const int z = (int)(row / H);
    const uint64_t* p = lab + row * W;
    int x = 0;
    while (x < W) {
      const uint64_t f = p[x];
      int len = 1;
      while (x + len < W && p[x + len] == f) ++len;
      x += len;
      if (!f) continue;
      if (f >= HTOMB) { atomicOr(&w.counters[3], 1u); continue; }
      uint32_t s = (uint32_t)mix64(f) & (w.icap - 1);
      bool ok = false;
      for (uint32_t probe = 0; probe < w.icap; ++probe) {
        const unsigned long long old = atomicCAS((unsigned long long*)&w.idkeys[s], HEMPTY, f);
        if (old == HEMPTY) {
          if (atomicAdd(&w.counters[0], 1u) >= w.node_cap) atomicOr(&w.counters[3], 2u);
          ok = true;
          break;
        }
        if (old == f) { ok = true; break; }
        s = (s + 1) & (w.icap - 1);
      }
      if (!ok) { atomicOr(&w.counters[3], 2u); continue; }
      atomicAdd(&w.tcount[s], (unsigned long long)len);
      atomicMin(&w.tzmin[s], z0 + z);
      atomicMax(&w.tzmax[s], z0 + z);
    }
  }
}

__global__ void ltab_compact_kernel(AggWs w) {
  if (w.counters[3]) return;
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < w.icap; s += gridDim.x * blockDim.x) {
    if (w.idkeys[s] == HEMPTY) continue;
    const uint32_t i = atomicAdd(&w.counters[1], 1u);
    if (i < w.node_cap) {
      w.idu[i] = w.idkeys[s];
      w.ha[i] = s;
    }
  }
}

__global__ void ltab_pad_kernel(AggWs w) {
  const uint32_t nn = min(w.counters[0], w.node_cap);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < w.node_cap; i += gridDim.x * blockDim.x)
    if (i >= nn) { w.idu[i] = HEMPTY; w.ha[i] = 0; }
}

__global__ void ltab_gather_kernel(AggWs w, uint64_t* __restrict__ ids, uint64_t* __restrict__ counts, int32_t* __restrict__ zmin,
                                   int32_t* __restrict__ zmax, uint64_t cap, uint64_t* __restrict__ n_out) {
  keep_overflow(w);
  if (w.counters[3]) return;
  const uint32_t nn = w.counters[0];
  if (nn > cap) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { atomicOr(&w.counters[3], 32u); atomicOr(w.sticky, 32u); }
    return;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *n_out = nn;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nn; i += gridDim.x * blockDim.x) {
    const uint32_t s = w.hb[i];
    ids[i] = w.ids[i];
    counts[i] = w.tcount[s];
    zmin[i] = w.tzmin[s];
    zmax[i] = w.tzmax[s];
  }
}

// per-label voxel count and coordinate sums (RAG node attributes, watershed_frags.py:230-246)
__device__ __forceinline__ void label_stats_body(const uint64_t* __restrict__ lab, int D, int H, int W, uint64_t id_offset, uint64_t num,
                                   unsigned long long* __restrict__ size, unsigned long long* __restrict__ sums) {
  const size_t n = (size_t)D * H * W;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const uint64_t l = lab[p];
    if (l <= id_offset || l - id_offset > num) continue;
    const uint64_t k = l - id_offset - 1;
    atomicAdd(&size[k], 1ull);
    atomicAdd(&sums[3 * k + 0], (unsigned long long)(p / ((size_t)W * H)));
    atomicAdd(&sums[3 * k + 1], (unsigned long long)((p / W) % H));
    atomicAdd(&sums[3 * k + 2], (unsigned long long)(p % W));
  }
}
__global__ void label_stats_kernel(const uint64_t* __restrict__ lab, int D, int H, int W, uint64_t id_offset, uint64_t num,
                                   unsigned long long* __restrict__ size, unsigned long long* __restrict__ sums) { label_stats_body(lab, D, H, W, id_offset, num, size, sums); }
__global__ void label_stats_batch_kernel(const BatchBlock* __restrict__ tab, int D, int H, int W, uint64_t num) {
  const BatchBlock& b = tab[blockIdx.y];
  label_stats_body(b.f.labels, D, H, W, b.f.id_offset, num, (unsigned long long*)b.f.size, (unsigned long long*)b.f.sums);
}

// bsmi_frag_postprocess_u8 and bsmi_label_stats (below) for rows 0..N-1 of the table, one launch per kernel.  The fills of both
// (flags, the filter's tables, the statistics' outputs) are the rows' `fills`: the caller has launched them.
void batch_post_launch(const BatchBlock* tab, int N, const int64_t shape[3], double filter_value, int64_t min_size, const int64_t crop_offset[3],
                       const int64_t crop_shape[3], uint64_t stats_num, hipStream_t s) {
  const size_t n = (size_t)shape[0] * shape[1] * shape[2];
  const size_t nc = (size_t)crop_shape[0] * crop_shape[1] * crop_shape[2];
  const int bs = 256;
  const dim3 grid((unsigned)std::min<size_t>((n + bs - 1) / bs, 4096), N);
  const dim3 gridc((unsigned)std::min<size_t>((nc + bs - 1) / bs, 4096), N);
  if (filter_value > 0.0 || min_size > 0) {
    hipLaunchKernelGGL(frag_stats_batch_kernel, grid, dim3(bs), 0, s, tab, n);
    hipLaunchKernelGGL(frag_decide_batch_kernel, grid, dim3(bs), 0, s, tab, n, filter_value, (long long)min_size);
    hipLaunchKernelGGL(frag_filter_batch_kernel, grid, dim3(bs), 0, s, tab, n);
  }
  const int cd = (int)crop_shape[0], ch = (int)crop_shape[1], cw = (int)crop_shape[2];
  hipLaunchKernelGGL(crop_u64_batch_kernel, gridc, dim3(bs), 0, s, tab, (int)shape[1], (int)shape[2], (int)crop_offset[0], (int)crop_offset[1],
                     (int)crop_offset[2], cd, ch, cw);
  hipLaunchKernelGGL(cc26_init_batch_kernel, gridc, dim3(bs), 0, s, tab, nc);
  hipLaunchKernelGGL(cc26_union_batch_kernel, gridc, dim3(bs), 0, s, tab, cd, ch, cw);
  const uint32_t nblk = (uint32_t)((nc + 1023) / 1024);
  hipLaunchKernelGGL(cc26_count_batch_kernel, dim3(nblk, N), dim3(1024), 0, s, tab, nc);
  hipLaunchKernelGGL(cc26_scan_batch_kernel, dim3(1, N), dim3(1024), 0, s, tab, nblk);
  hipLaunchKernelGGL(cc26_rank_batch_kernel, dim3(nblk, N), dim3(1024), 0, s, tab, nc);
  hipLaunchKernelGGL(cc26_write_batch_kernel, gridc, dim3(bs), 0, s, tab, nc);
  hipLaunchKernelGGL(label_stats_batch_kernel, gridc, dim3(bs), 0, s, tab, cd, ch, cw, stats_num);
}

}  // namespace bsmi

using namespace bsmi;

extern "C" {

int bsmi_frag_postprocess_u8(bsmi_seg* h, const uint8_t* affs_dev, uint64_t* frags_dev, const int64_t shape[3],
                             double filter_value, int64_t min_size, const int64_t crop_offset[3],
                             const int64_t crop_shape[3], uint64_t id_offset, uint64_t* out_dev, uint64_t* num_labels_dev,
                             void* stream) {
  int rc = check_seg_shape(h, shape);
  if (rc) return rc;
  if (!affs_dev || !frags_dev || !crop_offset || !crop_shape || !out_dev || !num_labels_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  for (int d = 0; d < 3; ++d)
    if (crop_offset[d] < 0 || crop_shape[d] < 1 || crop_offset[d] + crop_shape[d] > shape[d])
      BSMI_FAIL(BSMI_ERR_INVALID, "crop outside the fragment volume");
  BSMI_HIP(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)shape[0] * shape[1] * shape[2];
  const size_t nc = (size_t)crop_shape[0] * crop_shape[1] * crop_shape[2];
  FragWs& f = h->frag;
  const int bs = 256;
  const int grid = (int)std::min<size_t>((n + bs - 1) / bs, 4096);
  const int gridc = (int)std::min<size_t>((nc + bs - 1) / bs, 4096);
  {
    Fills fl;
    fl.add(f.flags, 4 * sizeof(uint32_t));
    if (filter_value > 0.0 || min_size > 0) {
      fl.add(f.lsum, (size_t)f.id_cap * sizeof(unsigned long long));
      fl.add(f.lcnt, (size_t)f.id_cap * sizeof(uint32_t));
    }
    fl.launch(s);
  }
  if (filter_value > 0.0 || min_size > 0) {
    hipLaunchKernelGGL(frag_stats_kernel, dim3(grid), dim3(bs), 0, s, affs_dev, (const uint64_t*)frags_dev, n, f);
    hipLaunchKernelGGL(frag_decide_kernel, dim3(grid), dim3(bs), 0, s, affs_dev, (const uint64_t*)frags_dev, n, f, filter_value,
                       (long long)min_size);
    hipLaunchKernelGGL(frag_filter_kernel, dim3(grid), dim3(bs), 0, s, frags_dev, n, f);
  }
  hipLaunchKernelGGL(crop_u64_kernel, dim3(gridc), dim3(bs), 0, s, (const uint64_t*)frags_dev, (int)shape[1], (int)shape[2],
                     (int)crop_offset[0], (int)crop_offset[1], (int)crop_offset[2], (int)crop_shape[0], (int)crop_shape[1],
                     (int)crop_shape[2], h->crop_tmp);
  hipLaunchKernelGGL(cc26_init_kernel, dim3(gridc), dim3(bs), 0, s, (const uint64_t*)h->crop_tmp, nc, f);
  hipLaunchKernelGGL(cc26_union_kernel, dim3(gridc), dim3(bs), 0, s, (const uint64_t*)h->crop_tmp, (int)crop_shape[0],
                     (int)crop_shape[1], (int)crop_shape[2], f);
  cc_rank_roots(nc, f, num_labels_dev, s);
  hipLaunchKernelGGL(cc26_write_kernel, dim3(gridc), dim3(bs), 0, s, (const uint64_t*)h->crop_tmp, nc, f, id_offset, out_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_label_stats(bsmi_seg* h, const uint64_t* labels_dev, const int64_t shape[3], uint64_t id_offset, uint64_t num,
                     uint64_t* size_dev, uint64_t* sums_dev, void* stream) {
  int rc = check_seg_shape(h, shape);
  if (rc) return rc;
  if (!labels_dev || !size_dev || !sums_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  BSMI_HIP(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)shape[0] * shape[1] * shape[2];
  {
    Fills fl;
    fl.add(size_dev, num * sizeof(uint64_t));
    fl.add(sums_dev, 3 * num * sizeof(uint64_t));
    fl.launch(s);
  }
  const int bs = 256;
  hipLaunchKernelGGL(label_stats_kernel, dim3((int)std::min<size_t>((n + bs - 1) / bs, 4096)), dim3(bs), 0, s, labels_dev,
                     (int)shape[0], (int)shape[1], (int)shape[2], id_offset, num, (unsigned long long*)size_dev,
                     (unsigned long long*)sums_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_lut_relabel(int device, const uint64_t* in_dev, uint64_t n, const uint64_t* keys_dev, const uint64_t* vals_dev, uint64_t m,
                     uint64_t* out_dev, void* stream) {
  if (!in_dev || !out_dev || (m && (!keys_dev || !vals_dev))) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  BSMI_HIP(hipSetDevice(device));
  if (!n) return BSMI_OK;
  const int bs = 256;
  hipLaunchKernelGGL(lut_relabel_kernel, dim3((int)std::min<uint64_t>((n + bs - 1) / bs, 8192)), dim3(bs), 0, (hipStream_t)stream,
                     in_dev, (size_t)n, keys_dev, vals_dev, m, out_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_lut_relabel_multi(int device, const uint64_t* in_dev, uint64_t n, const uint64_t* keys_dev, const uint64_t* vals_dev, uint64_t m,
                           int n_columns, uint64_t* out_dev, void* stream) {
  if (!in_dev || !out_dev || (m && (!keys_dev || !vals_dev))) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (n_columns < 1 || n_columns > kLutMaxColumns) BSMI_FAIL(BSMI_ERR_INVALID, "1 to %d value columns", kLutMaxColumns);
  BSMI_HIP(hipSetDevice(device));
  if (!n) return BSMI_OK;
  LutColumns c{};
  for (int t = 0; t < n_columns; ++t) {
    c.vals[t] = vals_dev ? vals_dev + (size_t)t * m : nullptr;
    c.out[t] = out_dev + (size_t)t * n;
  }
  const int bs = 256;
  const uint64_t nruns = (n + 7) / 8;
  hipLaunchKernelGGL(lut_relabel_multi_kernel, dim3((int)std::min<uint64_t>((nruns + bs - 1) / bs, 16384)), dim3(bs), 0, (hipStream_t)stream,
                     in_dev, (size_t)n, keys_dev, m, n_columns, c);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_cc_affs_u8(bsmi_seg* h, const uint8_t* affs_dev, const int64_t shape[3], int cut, int64_t min_size, uint64_t* frags_dev,
                    uint64_t* seg_dev, uint64_t* num_labels_dev, void* stream) {
  int rc = check_seg_shape(h, shape);
  if (rc) return rc;
  if (!affs_dev || !frags_dev || !num_labels_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (cut < -1 || cut > 255) BSMI_FAIL(BSMI_ERR_INVALID, "cut must be in [-1, 255]");
  BSMI_HIP(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)shape[0] * shape[1] * shape[2];
  FragWs& f = h->frag;
  const int bs = 256;
  const int grid = (int)std::min<size_t>((n + bs - 1) / bs, 4096);
  BSMI_HIP(hipMemsetAsync(f.flags, 0, 4 * sizeof(uint32_t), s));
  hipLaunchKernelGGL(ccaff_init_kernel, dim3(grid), dim3(bs), 0, s, n, f, h->crop_tmp);
  hipLaunchKernelGGL(ccaff_union_kernel, dim3(grid), dim3(bs), 0, s, affs_dev, (int)shape[0], (int)shape[1], (int)shape[2], cut, f, h->crop_tmp);
  hipLaunchKernelGGL(ccaff_finalize_kernel, dim3(grid), dim3(bs), 0, s, n, f, (const uint64_t*)h->crop_tmp);
  cc_rank_roots(n, f, num_labels_dev, s);
  hipLaunchKernelGGL(cc26_write_kernel, dim3(grid), dim3(bs), 0, s, (const uint64_t*)h->crop_tmp, n, f, (uint64_t)0, frags_dev);
  if (seg_dev) {
    BSMI_HIP(hipMemcpyAsync(seg_dev, frags_dev, n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    if (min_size > 0) {  // skimage remove_small_objects on the labels (post/connected_components.py:97-101)
      BSMI_HIP(hipMemsetAsync(f.lsum, 0, (size_t)f.id_cap * sizeof(unsigned long long), s));
      BSMI_HIP(hipMemsetAsync(f.lcnt, 0, (size_t)f.id_cap * sizeof(uint32_t), s));
      hipLaunchKernelGGL(frag_stats_kernel, dim3(grid), dim3(bs), 0, s, affs_dev, (const uint64_t*)seg_dev, n, f);
      hipLaunchKernelGGL(frag_decide_kernel, dim3(grid), dim3(bs), 0, s, affs_dev, (const uint64_t*)seg_dev, n, f, 0.0, (long long)min_size);
      hipLaunchKernelGGL(frag_filter_kernel, dim3(grid), dim3(bs), 0, s, seg_dev, n, f);
    }
  }
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_label_table_u64(bsmi_seg* h, const uint64_t* labels_dev, const int64_t shape[3], int64_t z0, uint64_t* ids_dev, uint64_t* counts_dev,
                         int32_t* zmin_dev, int32_t* zmax_dev, uint64_t capacity, uint64_t* n_dev, void* stream) {
  int rc = check_seg_shape(h, shape);
  if (rc) return rc;
  if (!labels_dev || !ids_dev || !counts_dev || !zmin_dev || !zmax_dev || !n_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  BSMI_HIP(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  AggWs& g = h->agg;
  const int D = (int)shape[0], H = (int)shape[1], W = (int)shape[2];
  BSMI_HIP(hipMemsetAsync(g.counters, 0, 8 * sizeof(uint32_t), s));
  BSMI_HIP(hipMemsetAsync(n_dev, 0, sizeof(uint64_t), s));
  hipLaunchKernelGGL(ltab_clear_kernel, dim3(512), dim3(256), 0, s, g);
  const size_t nrows = (size_t)D * H;
  hipLaunchKernelGGL(ltab_scan_kernel, dim3((unsigned)std::min<size_t>((nrows + 63) / 64, 8192)), dim3(64), 0, s, labels_dev, D, H, W, (int)z0, g);
  hipLaunchKernelGGL(ltab_compact_kernel, dim3(512), dim3(256), 0, s, g);
  hipLaunchKernelGGL(ltab_pad_kernel, dim3(256), dim3(256), 0, s, g);
  BSMI_HIP(seg_sort_pairs_u64_u32(h->sort_tmp, h->sort_tmp_bytes, g.idu, g.ids, g.ha, g.hb, (int)g.node_cap, s));
  hipLaunchKernelGGL(ltab_gather_kernel, dim3(256), dim3(256), 0, s, g, ids_dev, counts_dev, zmin_dev, zmax_dev, capacity, n_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

}  // extern "C"

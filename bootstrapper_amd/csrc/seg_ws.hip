// Watershed fragments, fragments_in_xy mode (reference post/ws.py:8-95): seeds per slice, the id offsets, and the three forms
// of the per-slice flood (compact record, plain, wide for slices of 2^20 voxels and more); the public fragments entry, which
// hands the 3-D mode to seg_ws3.hip.
#include "seg_internal.h"

#include "dev_guard.h"  // last: routes hipMalloc / hipFree through the guarded allocator (BSMI_GUARD_MB)

namespace bsmi {

constexpr int WS_T = 1024;           // threads per slice workgroup (seeds kernel): 16 waves, so that its LDS loops hide their latency
#ifndef BSMI_FLOOD_WAVES
#define BSMI_FLOOD_WAVES 8
#endif
// slices per flood workgroup (one wave each).  8, i.e. 20 workgroups of 64 KB of LDS per 160-slice block, two to a CU: with the
// stages run one after the other (the default) the chip is the lanes' alone, and spread over twice the CUs the floods of 20
// blocks side by side finish in 32 ms where 16 waves per workgroup took 41 (4 waves: as 8).  16 suited the overlapped mode, where
// a flood workgroup keeps a convolution workgroup off its CU.
constexpr int FLOOD_WAVES = BSMI_FLOOD_WAVES;
constexpr int FLOOD_LDS_HEAP = 1024; // heap entries per slice kept in LDS (8 B each); the rest spills to HBM

// LDS = true: the row distances / filter intermediates (uint16) and the squared distances
// (int32) of the slice live in LDS ([H][W+2] uint16 + [H*W] int32, <= 160 KiB for slices up to
// 160 x 160); LDS = false: same algorithm on the global scratch arrays (any slice size).
template <bool LDS>
__device__ __forceinline__ void ws_seeds_body(const uint8_t* __restrict__ affs, int D, int H, int W, int msd, const WsScratch& s,
                                              int compact) {
  extern __shared__ __attribute__((aligned(16))) char ws_smem[];
  const int z = blockIdx.x;
  const int n = H * W;
  const size_t vol = (size_t)D * n;
  const uint8_t* ay = affs + vol + (size_t)z * n;
  const uint8_t* ax = affs + 2 * vol + (size_t)z * n;
  uint8_t* mask = s.mask + (size_t)z * n;
  int32_t* g = s.g + (size_t)z * n;
  int32_t* d2 = s.d2 + (size_t)z * n;
  int32_t* mf = s.mf + (size_t)z * n;
  int32_t* par = s.par + (size_t)z * n;
  int32_t* lab = s.lab + (size_t)z * n;
  const int tid = threadIdx.x;
  __shared__ int sh_any_bg;
  __shared__ int sh_wave[WS_T / 64];
  const bool near = msd <= H && msd <= W;  // the maximum filter's window reflects at most once
  if (tid == 0) sh_any_bg = 0;
  __syncthreads();
  // The sequential per-row loops below (row distances, run labelling, numbering) must not walk global memory: a load
  // per step and row, 160 steps, at the L2 latency of a busy chip made a slice's workgroup -- which holds a whole CU's LDS --
  // live 0.6 ms, 6.4 ms per block under 16 lanes.  So the LDS path keeps what those loops read in LDS: the mask, and a
  // flag byte per voxel (is a maximum / is a root).  LDS: sg u16 [H][W+2] | sd2 u16 [H*W] | smask u8 [H*W] | sflag u8 [H*W].
  uint8_t* smask = nullptr;
  uint8_t* sflag = nullptr;
  const uint16_t* sd2_lds = nullptr;
  // compact (LDS path only): the flood's state of a voxel is ONE 32-bit record in `lab` -- marker label | squared distance << 16,
  // inside the mask <=> distance > 0 -- instead of three arrays (see ws_flood_kernel); mask and d2 then stay out of HBM
  if constexpr (!LDS) compact = 0;
  if constexpr (LDS) {
    const size_t o_sd2 = ((size_t)H * (W + 2) * 2 + 15) & ~(size_t)15;
    sd2_lds = (const uint16_t*)(ws_smem + o_sd2);
    const size_t o_mask = (o_sd2 + (size_t)n * 2 + 15) & ~(size_t)15;
    smask = (uint8_t*)(ws_smem + o_mask);
    sflag = smask + (((size_t)n + 15) & ~(size_t)15);
  }
  // a. mask  (0.5*(a_y+a_x) > 0.5*255  <=>  a_y + a_x >= 256)
  int bg = 0;
  for (int i = tid; i < n; i += WS_T) {
    const int m = (int)ay[i] + (int)ax[i] >= 256;
    if (!compact) mask[i] = (uint8_t)m;
    if constexpr (LDS) smask[i] = (uint8_t)m;
    bg |= !m;
  }
  if (bg) sh_any_bg = 1;
  __syncthreads();
  const int any_bg = sh_any_bg;
  constexpr int INF = 1 << 28;
  if constexpr (LDS) {
    // ---- LDS path: sg = row distances, later the x-filtered d2 (all values < 65535) ----------
    const int Wp = W + 2;  // row stride in uint16: consecutive rows fall into different banks
    uint16_t* sg = (uint16_t*)ws_smem;
    uint16_t* sd2 = (uint16_t*)(ws_smem + (((size_t)H * Wp * 2 + 15) & ~(size_t)15));  // squared distances < 65535 (launcher)
    constexpr int GINF = 0xffff;
    if (any_bg) {
      for (int y = tid; y < H; y += WS_T) {
        int last = -INF;
        for (int x = 0; x < W; ++x) {
          if (!smask[y * W + x]) last = x;
          sg[y * Wp + x] = (uint16_t)(last <= -INF ? GINF : x - last);
        }
        last = INF;
        for (int x = W - 1; x >= 0; --x) {
          if (!smask[y * W + x]) last = x;
          const int d = last >= INF ? GINF : last - x;
          if (d < (int)sg[y * Wp + x]) sg[y * Wp + x] = (uint16_t)d;
        }
      }
      __syncthreads();
      for (int i = tid; i < n; i += WS_T) {
        const int y = i / W, x = i - y * W;
        // min over rows of g(row, x)^2 + (y - row)^2, outwards from the own row: a row k away cannot improve on a best <= k^2
        const int g0 = sg[y * Wp + x];
        int best = g0 == GINF ? INF : g0 * g0;
        for (int k = 1; k < H && k * k < best; ++k) {
          if (y - k >= 0) {
            const int gg = sg[(y - k) * Wp + x];
            const int v = gg == GINF ? INF : gg * gg + k * k;
            best = v < best ? v : best;
          }
          if (y + k < H) {
            const int gg = sg[(y + k) * Wp + x];
            const int v = gg == GINF ? INF : gg * gg + k * k;
            best = v < best ? v : best;
          }
        }
        sd2[i] = (uint16_t)best;
        if (!compact) d2[i] = best;
      }
    } else {
      for (int i = tid; i < n; i += WS_T) {
        const int y = i / W, x = i - y * W;
        const int v = (y + 1) * (y + 1) + x * x;
        sd2[i] = (uint16_t)v;
        if (!compact) d2[i] = v;
      }
    }
    __syncthreads();
    const int left = msd / 2, right = msd - 1 - msd / 2;
    for (int i = tid; i < n; i += WS_T) {
      const int y = i / W, x = i - y * W;
      int m = INT32_MIN;
      for (int k = x - left; k <= x + right; ++k) {
        const int v = sd2[y * W + (near ? reflect_near(k, W) : reflect_dup(k, W))];
        m = v > m ? v : m;
      }
      sg[y * Wp + x] = (uint16_t)m;
    }
    __syncthreads();
    for (int i = tid; i < n; i += WS_T) {
      const int y = i / W, x = i - y * W;
      int m = INT32_MIN;
      for (int k = y - left; k <= y + right; ++k) {
        const int v = sg[(near ? reflect_near(k, H) : reflect_dup(k, H)) * Wp + x];
        m = v > m ? v : m;
      }
      sflag[i] = (uint8_t)(m == (int)sd2[i]);   // d. is this voxel a maximum of the filtered distance?
    }
    __syncthreads();
  } else {
  if (any_bg) {
    // b1. per row: distance along x to the nearest background voxel
    for (int y = tid; y < H; y += WS_T) {
      int last = -INF;
      for (int x = 0; x < W; ++x) {
        if (!mask[y * W + x]) last = x;
        g[y * W + x] = last <= -INF ? INF : x - last;
      }
      last = INF;
      for (int x = W - 1; x >= 0; --x) {
        if (!mask[y * W + x]) last = x;
        const int d = last >= INF ? INF : last - x;
        if (d < g[y * W + x]) g[y * W + x] = d;
      }
    }
    __syncthreads();
    // b2. per voxel: min over y' of g(y',x)^2 + (y-y')^2   (exact, integers)
    if (n >= (1 << 20)) {
      // full-size sections: outwards from the own row, as the LDS path does -- a row k away cannot improve on a best <= k^2,
      // so a voxel walks O(distance) rows instead of H (the same minimum; a 1250^2 slice with one straight edge, distances up
      // to 625: the kernel 645 -> 108 ms)
      for (int i = tid; i < n; i += WS_T) {
        const int y = i / W;
        const int g0 = g[i];
        int best = g0 < INF ? g0 * g0 : INF;
        for (int k = 1; k < H && k * k < best; ++k) {
          if (y - k >= 0) {
            const int gg = g[i - k * W];
            const int v = gg < INF ? gg * gg + k * k : INF;
            best = v < best ? v : best;
          }
          if (y + k < H) {
            const int gg = g[i + k * W];
            const int v = gg < INF ? gg * gg + k * k : INF;
            best = v < best ? v : best;
          }
        }
        d2[i] = best;
      }
    } else
    for (int i = tid; i < n; i += WS_T) {
      const int y = i / W, x = i - y * W;
      int best = INF;
      for (int yy = 0; yy < H; ++yy) {
        const int gg = g[yy * W + x];
        if (gg < INF) {
          const int dy = y - yy;
          const int v = gg * gg + dy * dy;
          best = v < best ? v : best;
        }
      }
      d2[i] = best;
    }
  } else {
    // scipy's behaviour without any background voxel: as if the only one sat at (-1, 0)
    for (int i = tid; i < n; i += WS_T) {
      const int y = i / W, x = i - y * W;
      d2[i] = (y + 1) * (y + 1) + x * x;
    }
  }
  __syncthreads();
  // c. maximum_filter(size=msd), window [i - msd/2, i + msd - 1 - msd/2], reflect border
  const int left = msd / 2, right = msd - 1 - msd / 2;
  for (int i = tid; i < n; i += WS_T) {
    const int y = i / W, x = i - y * W;
    int m = INT32_MIN;
    for (int k = x - left; k <= x + right; ++k) {
      const int v = d2[y * W + (near ? reflect_near(k, W) : reflect_dup(k, W))];
      m = v > m ? v : m;
    }
    g[i] = m;
  }
  __syncthreads();
  for (int i = tid; i < n; i += WS_T) {
    const int y = i / W, x = i - y * W;
    int m = INT32_MIN;
    for (int k = y - left; k <= y + right; ++k) {
      const int v = g[(near ? reflect_near(k, H) : reflect_dup(k, H)) * W + x];
      m = v > m ? v : m;
    }
    mf[i] = m;
  }
  __syncthreads();
  }
  // d/e. maxima and their 4-connected components.  Rows are labelled as runs first (each
  // maximum points at the first voxel of its run), then vertically adjacent runs are united
  // once, at the first column where they overlap (union-find, smaller index wins).
  for (int y = tid; y < H; y += WS_T) {
    int start = -1;
    for (int x = 0; x < W; ++x) {
      const int i = y * W + x;
      bool is_max;
      if constexpr (LDS) is_max = sflag[i] != 0;
      else is_max = mf[i] == d2[i];
      if (is_max) {
        if (start < 0) start = i;
        par[i] = start;
      } else {
        par[i] = -1;
        start = -1;
      }
    }
  }
  __syncthreads();
  auto find = [&](int a) {
    int p = par[a];
    while (p != a) {
      a = p;
      p = __hip_atomic_load(&par[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    return a;
  };
  auto unite = [&](int a, int b) {
    for (;;) {
      a = find(a);
      b = find(b);
      if (a == b) return;
      if (a < b) { const int t = a; a = b; b = t; }
      const int old = atomicMin(&par[a], b);
      if (old == a) return;
      a = old;
    }
  };
  for (int i = tid; i < n; i += WS_T) {
    if (i < W || par[i] < 0 || par[i - W] < 0) continue;
    const int x = i % W;
    if (x > 0 && par[i - 1] >= 0 && par[i - W - 1] >= 0) continue;  // this run pair was united further left
    unite(i, i - W);
  }
  __syncthreads();
  // raster-order numbering of the roots (scipy.ndimage.label): chunked scan (LDS path: over root flags gathered by a
  // coalesced pass, not over the global parent array element by element)
  if constexpr (LDS) {
    for (int i = tid; i < n; i += WS_T) sflag[i] = (uint8_t)(par[i] == i);
    __syncthreads();
  }
  const int chunk = (n + WS_T - 1) / WS_T;
  const int c0 = tid * chunk, c1 = min(n, c0 + chunk);
  int cnt = 0;
  for (int i = c0; i < c1; ++i) {
    if constexpr (LDS) cnt += sflag[i];
    else cnt += (par[i] == i);
  }
  // exclusive scan of the chunk counts over the workgroup's threads: in a wave by shuffles, the 16 wave totals by wave 0
  const int lane = tid & 63, wave = tid >> 6;
  int incl = cnt;
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  if (lane == 63) sh_wave[wave] = incl;
  __syncthreads();
  if (wave == 0) {
    int w = lane < WS_T / 64 ? sh_wave[lane] : 0;
    for (int o = 1; o < WS_T / 64; o <<= 1) {
      const int t = __shfl_up(w, o);
      if (lane >= o) w += t;
    }
    if (lane < WS_T / 64) sh_wave[lane] = w;
  }
  __syncthreads();
  int id = (wave ? sh_wave[wave - 1] : 0) + incl - cnt;
  if (tid == WS_T - 1) s.nseeds[z] = id + cnt;
  for (int i = c0; i < c1; ++i) {
    bool root;
    if constexpr (LDS) root = sflag[i] != 0;
    else root = par[i] == i;
    if (root) g[i] = ++id;  // g reused: root index -> label
  }
  __syncthreads();
  // markers = label * mask (seeds outside the mask vanish inside skimage)
  for (int i = tid; i < n; i += WS_T) {
    int l = 0;
    if (par[i] >= 0) {
      const int sl = g[find(i)];
      if (s.seedlab) s.seedlab[(size_t)z * n + i] = sl;
      bool inside;
      if constexpr (LDS) inside = smask[i] != 0;
      else inside = mask[i] != 0;
      if (inside) l = sl;
    } else if (s.seedlab) {
      s.seedlab[(size_t)z * n + i] = 0;
    }
    if (compact) ((uint32_t*)lab)[i] = (uint32_t)l | ((uint32_t)sd2_lds[i] << 16);
    else lab[i] = l;
  }
}
template <bool LDS>
__global__ __launch_bounds__(WS_T) void ws_seeds_kernel(const uint8_t* __restrict__ affs, int D, int H, int W,
                                                        int msd, WsScratch s, int compact) {
  ws_seeds_body<LDS>(affs, D, H, W, msd, s, compact);
}
// batched form (LDS / compact path): block blockIdx.y of the table, slice blockIdx.x
__global__ __launch_bounds__(WS_T) void ws_seeds_batch_kernel(const BatchBlock* __restrict__ tab, int D, int H, int W, int msd, int compact) {
  const BatchBlock& b = tab[blockIdx.y];
  ws_seeds_body<true>(b.f.affs, D, H, W, msd, b.ws, compact);
}

__device__ __forceinline__ void ws_offsets_body(int D, const WsScratch& s, uint64_t* max_id) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    uint64_t acc = 0;
    for (int z = 0; z < D; ++z) { s.offs[z] = acc; acc += (uint64_t)s.nseeds[z]; }
    *max_id = acc;
  }
}
__global__ void ws_offsets_kernel(int D, WsScratch s, uint64_t* max_id) { ws_offsets_body(D, s, max_id); }
__global__ void ws_offsets_batch_kernel(const BatchBlock* __restrict__ tab, int D) {
  const BatchBlock& b = tab[blockIdx.y];
  ws_offsets_body(D, b.ws, b.f.max_id);
}

// lane 0's 64-bit value to the whole wave
__device__ __forceinline__ uint64_t bcast0(uint64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}

// heap entry: [63:40] = MAXD2 - d2 (24 bit) | [39:20] = age (20 bit) | [19:0] = voxel index.
// Ordering ignores the index bits (skimage compares (value, age) only).
// (The scalar unit, where the wave-uniform flood loop runs, has no 64-bit ordered compare; a vector compare and the trip of its
// result back to a scalar register are ten instructions, and the floods of a stage's blocks side by side are bound by
// instruction issue.  The sign of the difference of the two 44-bit keys is scalar work: two shifts, a subtract with borrow.)
__device__ __forceinline__ bool flood_smaller(uint64_t a, uint64_t b) { return (int64_t)((a >> 20) - (b >> 20)) < 0; }

// COMPACT: a voxel's state is the 32-bit record ws_seeds_kernel leaves in `lab` (label | squared distance << 16; in the mask <=>
// distance > 0): a pop touches three cache lines (the rows above, of and below the voxel) instead of nine, and a slice is 100 KB
// instead of 230 -- side by side, the floods of a stage's blocks are bound by the lines they pull through L2, not by one wave's
// latency chain.
template <bool COMPACT>
__device__ __forceinline__ void ws_flood_body(int D, int H, int W, const WsScratch& s, uint64_t* heap_spill, size_t spill_stride,
                                              uint64_t* __restrict__ frags, int* status) {
  __shared__ uint64_t hl_all[FLOOD_WAVES][FLOOD_LDS_HEAP];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int z = blockIdx.x * FLOOD_WAVES + wave;
  if (z >= D) return;  // whole wave exits; no workgroup barrier is used below
  uint64_t* hl = hl_all[wave];
  const int n = H * W;
  const uint8_t* mask = s.mask + (size_t)z * n;
  const int32_t* d2 = s.d2 + (size_t)z * n;
  int32_t* lab = s.lab + (size_t)z * n;
  uint64_t* hg = heap_spill + (size_t)z * spill_stride;  // entries >= FLOOD_LDS_HEAP live here
  // The queue order is inherently sequential, so the whole wave walks the same loop in lockstep (every lane holds the
  // same `items`, `age` and heap values; lane 0 alone owns the heap).  What the other lanes buy: the four neighbours
  // of a popped voxel are fetched side by side -- lane k reads mask, label and distance of neighbour k in one round of
  // loads -- where a single lane would chain up to twelve dependent global loads per voxel.  Label stores are issued by
  // all four fetching lanes (same address, same value), so that each lane's later loads follow its own stores in program
  // order.
  // The compiler must KNOW that the loop is uniform: every value that comes out of memory goes through v_readfirstlane /
  // v_readlane (bcast0, uni), so that counters, heap indices and comparison results live in scalar registers and the loops
  // branch on the scalar unit.  Left to its divergence analysis it guarded each `if` of the sift loops with exec-mask
  // save / restore sequences -- about 100 instructions per heap level, 1000 per pop -- and the floods of a stage's blocks,
  // three waves to a SIMD, paid for it in instruction issue (20 blocks side by side: the last flood ends after 25.6 ms instead of 29.3).
  {
    constexpr uint64_t MAXD2 = (1u << 24) - 1;
    auto uni = [](int v) { return __builtin_amdgcn_readfirstlane(v); };
    // queue entry: [63:40] MAXD2 - d2 | [39:20] age | [19:0] voxel.  COMPACT (d2 < 2^16, fewer than 2^15 voxels, so fewer pushes):
    // [63:48] 65535 - d2 | [47:32] age | [31:16] label | [15:0] voxel -- the same order, the whole key is the upper word (one
    // scalar compare), and the label the voxel was given travels with it: a pop does not read the voxel's own record
    auto entry = [](uint64_t dd, uint32_t age_, uint64_t q_, uint32_t lbl_) -> uint64_t {
      return COMPACT ? ((65535ull - dd) << 48) | ((uint64_t)age_ << 32) | ((uint64_t)lbl_ << 16) | q_
                     : ((MAXD2 - dd) << 40) | ((uint64_t)age_ << 20) | q_;
    };
    auto smaller = [](uint64_t a_, uint64_t b_) -> bool {
      if constexpr (COMPACT) return (uint32_t)(a_ >> 32) < (uint32_t)(b_ >> 32);
      else return flood_smaller(a_, b_);
    };
    int items = 0;
    // the heap is written by lane 0 alone; its HBM spill is also read by lane 0 alone (and broadcast), so that those loads
    // follow that lane's stores in its own program order; LDS operations of a wave execute in order anyway
    // (Tried: the first 64 entries -- the six top levels every sift-down walks -- in registers, entry i in lane i, read with
    // v_readlane: fragments of a 128^3 block 12.7 -> 12.6 ms.  Also tried: label, distance and mask bit of a voxel packed into
    // one 8-byte record, five loads per pop instead of thirteen: 12.6 -> 11.8 ms alone, nothing under the pipeline's 16 lanes.)
    auto hget = [&](int i) -> uint64_t {
      if (i < FLOOD_LDS_HEAP) return hl[i];
      uint64_t v = 0;
      if (lane == 0) v = hg[i - FLOOD_LDS_HEAP];
      return bcast0(v);
    };
    auto hset = [&](int i, uint64_t v) {
      if (lane == 0) {
        if (i < FLOOD_LDS_HEAP) hl[i] = v; else hg[i - FLOOD_LDS_HEAP] = v;
      }
    };
    auto push = [&](uint64_t it) {
      int c = uni(items++);
      if constexpr (COMPACT) {
        if (c < FLOOD_LDS_HEAP) {  // (as below, with the key and the voxel of an entry as two 32-bit values; loads from a uniform LDS address are uniform to the compiler: no v_readfirstlane needed)
          const uint32_t ik = (uint32_t)(it >> 32), ix = (uint32_t)it;
          while (c > 0) {
            const int p = (c - 1) >> 1;
            const uint64_t pr = hl[p];
            const uint32_t pk = (uint32_t)(pr >> 32), px = (uint32_t)pr;
            if (!(ik < pk)) break;
            hl[c] = ((uint64_t)pk << 32) | px;
            c = p;
          }
          hl[c] = ((uint64_t)ik << 32) | ix;
          return;
        }
      }
      if (c < FLOOD_LDS_HEAP) {  // the whole path to the root is in LDS: no range checks per level
        while (c > 0) {
          const int p = (c - 1) >> 1;
          const uint64_t pv = hl[p];
          if (!smaller(it, pv)) break;
          hl[c] = pv;
          c = p;
        }
        hl[c] = it;
        return;
      }
      while (c > 0) {
        const int p = (c + 1) / 2 - 1;
        const uint64_t pv = hget(p);
        if (smaller(it, pv)) { hset(c, pv); c = uni(p); } else break;
      }
      hset(c, it);
    };
    // seeds in raster order, age 0
    uint32_t* rec = (uint32_t*)lab;
    for (int i0 = 0; i0 < n; i0 += 64) {
      const int i = i0 + lane;
      const int li = i < n ? (COMPACT ? (int)(rec[i] & 0xffffu) : lab[i]) : 0;
      unsigned long long seeds = __ballot(li != 0);
      while (seeds) {
        const int k = __ffsll(seeds) - 1;
        seeds &= seeds - 1;
        const int j = i0 + k;
        const uint32_t rj = COMPACT ? (uint32_t)uni((int)rec[j]) : 0u;
        const uint64_t dj = COMPACT ? (uint64_t)(rj >> 16) : (uint64_t)(uint32_t)uni(d2[j]);
        push(entry(dj, 0u, (uint64_t)j, rj & 0xffffu));
      }
    }
    uint32_t age = 0;
    const int k4 = lane & 3;
    const int dq = k4 == 0 ? -W : (k4 == 1 ? -1 : (k4 == 2 ? 1 : W));
    // y = idx / W without the division (idx < 2^20): exact for W < 4096 with the rounded-up reciprocal
    const bool rcp_ok = W > 1 && W < 4096;  // (W = 1: the reciprocal is 2^32)
    const uint32_t rcpW = (uint32_t)((((uint64_t)1 << 32) + (uint32_t)W - 1) / (uint32_t)W);
    // The pops run with lanes 0-3 alone (the four neighbour fetchers): inside, nothing is guarded by a lane test any more --
    // the heap writes of the LDS-only loops are issued by all active lanes (same address, same value) -- and the exec-mask
    // save / restore around every such write is gone.
    if (lane < 4)
    while (items > 0) {
      const uint64_t e = hget(0);
      --items;
      // the popped voxel's label and its neighbours' state are requested first: their latency hides behind the sift
      const int idx = COMPACT ? (int)((uint32_t)e & 0xffffu) : (int)(e & 0xfffffu);
      const int y = rcp_ok ? (int)__umulhi((uint32_t)idx, rcpW) : idx / W, x = idx - y * W;
      // neighbour order [-W, -1, +1, +W]: lane k < 4 looks at neighbour k; the other lanes stay out of global memory
      const bool okk = k4 == 0 ? y > 0 : (k4 == 1 ? x > 0 : (k4 == 2 ? x < W - 1 : y < H - 1));
      const int qk = okk ? idx + dq : idx;
      int lme = 0, mk = 0, lk = 0, dk = 0;
      {
        if constexpr (COMPACT) {
          const uint32_t rk = rec[qk];  // (a neighbour beyond the slice: the voxel's own record -- labelled, so no candidate)
          lme = (int)(((uint32_t)e >> 16) & 0xffffu);
          lk = (int)(rk & 0xffffu);
          dk = (int)(rk >> 16);
          mk = dk != 0;
        } else {
          lme = lab[idx];
          mk = mask[qk];
          lk = lab[qk];
          dk = d2[qk];
        }
      }
      if (items > 0) {
        // sift the last element down from the root (skimage heappop order)
        const uint64_t last = hget(items);
        int i = 0;
        // the levels whose two children both exist and live in LDS (all but the last one of a heap that fits): the smaller
        // child (the left one on a tie), then that one against `last` -- the same choice as the general form below makes
        const int lim = items < FLOOD_LDS_HEAP ? items : FLOOD_LDS_HEAP;
        bool placed = false;
        if constexpr (COMPACT) {  // (the loop below with the key and the voxel of an entry as two 32-bit values)
          const uint32_t lk = (uint32_t)(last >> 32);
          while (2 * i + 2 < lim) {
            const int c1 = 2 * i + 1;
            const uint64_t r1 = hl[c1], r2 = hl[c1 + 1];
            const uint32_t k1 = (uint32_t)(r1 >> 32), k2 = (uint32_t)(r2 >> 32);
            const uint32_t x1 = (uint32_t)r1, x2 = (uint32_t)r2;
            const bool right = k2 < k1;
            const uint32_t ck = right ? k2 : k1, cx = right ? x2 : x1;
            if (!(ck < lk)) { placed = true; break; }
            hl[i] = ((uint64_t)ck << 32) | cx;
            i = c1 + (right ? 1 : 0);
          }
        }
        while (!COMPACT && 2 * i + 2 < lim) {
          const int c1 = 2 * i + 1;
          const uint64_t r1 = hl[c1], r2 = hl[c1 + 1];
          const uint64_t v1 = r1, v2 = r2;
          const bool right = smaller(v2, v1);
          const uint64_t cv = right ? v2 : v1;
          if (!smaller(cv, last)) { placed = true; break; }
          hl[i] = cv;
          i = c1 + (right ? 1 : 0);
        }
        for (; !placed;) {
          const int c1 = 2 * i + 1, c2 = c1 + 1;
          if (c1 >= items) break;
          uint64_t v1, v2;
          if (c2 < FLOOD_LDS_HEAP) {  // both children with one LDS round trip (entry c2 = items is read and not looked at)
            const uint64_t r1 = hl[c1], r2 = hl[c2];
            v1 = r1;
            v2 = r2;
          } else {
            v1 = hget(c1);
            v2 = c2 < items ? hget(c2) : 0;
          }
          int sm = i;
          uint64_t smv = last;
          if (smaller(v1, smv)) { sm = c1; smv = v1; }
          if (c2 < items && smaller(v2, smv)) { sm = c2; smv = v2; }
          if (sm == i) break;
          hset(i, smv);
          i = uni(sm);
        }
        hset(i, last);
      }
      const int l = uni(lme);
      const bool cand = okk && mk && lk == 0;
      // the neighbours to take, in the order [-W, -1, +1, +W] (a voxel is taken once, so one per pop on average)
      for (uint32_t m = (uint32_t)__ballot(cand) & 0xfu; m; m &= m - 1) {
        const int k = __ffs((int)m) - 1;
        const int q = __builtin_amdgcn_readlane(qk, k);
        const uint64_t dd = (uint64_t)(uint32_t)__builtin_amdgcn_readlane(dk, k);
        ++age;
        if constexpr (COMPACT) rec[q] = (uint32_t)l | ((uint32_t)dd << 16);
        else lab[q] = l;
        push(entry(dd, age, (uint64_t)q, (uint32_t)l));
      }
    }
  }
  // the label writes become visible to the whole wave before the copy-out
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  const uint64_t off = s.offs[z];
  uint64_t* out = frags + (size_t)z * n;
  for (int i = lane; i < n; i += 64) {
    const int l = COMPACT ? (int)(((const uint32_t*)lab)[i] & 0xffffu) : lab[i];
    out[i] = l ? (uint64_t)l + off : 0ull;
  }
  (void)status;
}
template <bool COMPACT>
__global__ __launch_bounds__(64 * FLOOD_WAVES) void ws_flood_kernel(int D, int H, int W, WsScratch s, uint64_t* heap_spill,
                                                     size_t spill_stride, uint64_t* __restrict__ frags, int* status) {
  ws_flood_body<COMPACT>(D, H, W, s, heap_spill, spill_stride, frags, status);
}
// batched form (compact record): block blockIdx.y of the table, slices blockIdx.x * FLOOD_WAVES ... of it
__global__ __launch_bounds__(64 * FLOOD_WAVES) void ws_flood_batch_kernel(const BatchBlock* __restrict__ tab, int D, int H, int W) {
  const BatchBlock& b = tab[blockIdx.y];
  ws_flood_body<true>(D, H, W, b.ws, b.flood_spill, b.flood_spill_stride, b.f.frags, b.status);
}

// The flood of slices of 2^20 voxels and more (up to 4096 x 4096): ws_flood_kernel's packed entry has 20 bits for the age and
// the voxel.  Here an entry is a 64-bit key (MAXD2 - d2) << 32 | age -- the whole order, below 2^63, so that flood_smaller's
// trick (the sign of the difference) stays exact -- and a 32-bit voxel index beside it, in parallel arrays.  Same algorithm
// as ws_flood_kernel<false> and oracle/seg_ref.c:flood, bit for bit.
//
// One slice per workgroup (one wave): big slices come a few to a call, so a wave has a whole CU's LDS for the top
// FLOOD_WIDE_LDS_LEVELS levels of its heap (8191 entries, 96 KiB); deeper levels spill to HBM (`spill_key` / `spill_idx`,
// `spill_stride` entries per slice).  A blobby 1250^2 slice queues ~10^5 entries, so a sift-down usually ends 2-5 levels
// under the LDS part.  One round trip per spilled level would make it the loop's cost; instead, when the walk reaches the
// bottom LDS level, lanes 0-61 fetch the 62 entries of the next five levels under the current node in one round of loads
// (2 + 4 + 8 + 16 + 32), and the walk goes on through them with v_readlane.  Windows are rooted at depths 12, 17, 22, so
// every spilled node belongs to exactly one window, at one place in it: it has an owner lane, and ALL its global loads and
// stores -- window fetches, sift-down moves, sift-up reads and moves -- are issued by that lane alone.  A lane's accesses to
// an address follow its own program order, so no fence is needed between a store and a later window's load.
constexpr int FLOOD_WIDE_LDS_LEVELS = 13;
constexpr int FLOOD_WIDE_LDS_HEAP = (1 << FLOOD_WIDE_LDS_LEVELS) - 1;

// owner lane of spilled heap node i (i >= FLOOD_WIDE_LDS_HEAP): its depth below the window root k = 1..5 and position j in
// that level of the window -> lane 2^k - 2 + j
__device__ __forceinline__ int flood_wide_owner(uint32_t i) {
  const int d = 31 - __builtin_clz(i + 1);
  const int k = (d - FLOOD_WIDE_LDS_LEVELS) % 5 + 1;
  return (1 << k) - 2 + (int)((i + 1) & ((1u << k) - 1));
}

#ifdef BSMI_FLOOD_STATS  // dev build: where the wide flood's pops go, summed over slices (tools/probe_large_sections.py --stats)
// [0] pops  [1] sift-down moves within LDS  [2] window fetches  [3] sift-down moves within spilled levels  [4] pushes
// [5] sift-up moves  [6] sift-up parent reads from spilled levels  [7] `last` entries read from spilled levels
// [8] largest heap (max over slices)  [9] 100 MHz ticks of the pop loop  [10] slices
__device__ unsigned long long g_flood_stats[16];
extern "C" int bsmi_debug_flood_stats(unsigned long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_flood_stats), sizeof(unsigned long long) * 16) != hipSuccess) return -1;
  if (reset) {
    unsigned long long zero[16] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_flood_stats), zero, sizeof zero) != hipSuccess) return -1;
  }
  return 0;
}
#define FW_STAT(i, v) (st[i] += (v))
#else
#define FW_STAT(i, v) ((void)0)
#endif

__global__ __launch_bounds__(64) void ws_flood_wide_kernel(int D, int H, int W, WsScratch s, uint64_t* spill_key, uint32_t* spill_idx,
                                                           size_t spill_stride, uint64_t* __restrict__ frags) {
  constexpr int LH = FLOOD_WIDE_LDS_HEAP;
  __shared__ uint64_t hk[LH];
  __shared__ uint32_t hx[LH];
  const int lane = threadIdx.x;
  const int z = blockIdx.x;
  if (z >= D) return;
  const int n = H * W;
  const uint8_t* mask = s.mask + (size_t)z * n;
  const int32_t* d2 = s.d2 + (size_t)z * n;
  int32_t* lab = s.lab + (size_t)z * n;
  uint64_t* gk = spill_key + (size_t)z * spill_stride;  // gk[i - LH], gx[i - LH]: spilled node i (i >= LH)
  uint32_t* gx = spill_idx + (size_t)z * spill_stride;
  // the whole wave walks the one loop in lockstep, as in ws_flood_kernel: every value out of memory goes through
  // v_readfirstlane / v_readlane, so that the loop's control lives on the scalar unit
  {
    constexpr uint64_t MAXD2 = 0x7fffffffull;  // d2 <= 4096^2 + 4095^2 < 2^25 here (H, W <= 4096: launcher): keys < 2^63
    auto uni = [](int v) { return __builtin_amdgcn_readfirstlane(v); };
    auto rl64 = [](uint64_t v, int l) -> uint64_t {
      const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, l), hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
      return ((uint64_t)hi << 32) | lo;
    };
    auto smaller = [](uint64_t a_, uint64_t b_) -> bool { return (int64_t)(a_ - b_) < 0; };
    int items = 0;
#ifdef BSMI_FLOOD_STATS
    uint64_t st[11] = {};
    bool popping = false;
    uint64_t t0 = 0;
#endif
    // node i (LDS or spilled) -> wave-uniform key and index.  LDS writes are issued by every active lane (same address, same value).
    struct Ent { uint64_t k; uint32_t x; };
    auto hget = [gk, gx, lane, rl64](int i) -> Ent {
      if (i < LH) return {hk[i], hx[i]};
      const int o = flood_wide_owner((uint32_t)i);
      uint64_t kv = 0;
      uint32_t xv = 0;
      if (lane == o) { kv = gk[i - LH]; xv = gx[i - LH]; }
      return {rl64(kv, o), (uint32_t)__builtin_amdgcn_readlane((int)xv, o)};
    };
    auto hset = [gk, gx, lane](int i, uint64_t k_, uint32_t x_) {
      if (i < LH) { hk[i] = k_; hx[i] = x_; return; }
      if (lane == flood_wide_owner((uint32_t)i)) { gk[i - LH] = k_; gx[i - LH] = x_; }
    };
    auto push = [&](uint64_t ik, uint32_t ix) {
      int c = uni(items++);
#ifdef BSMI_FLOOD_STATS
      if (popping) FW_STAT(4, 1);
      if ((uint64_t)items > st[8]) st[8] = items;
#endif
      while (c > 0) {
        const int p = (c - 1) >> 1;
        const Ent pe = hget(p);
#ifdef BSMI_FLOOD_STATS
        if (popping && p >= LH) FW_STAT(6, 1);
#endif
        if (!smaller(ik, pe.k)) break;
        hset(c, pe.k, pe.x);
#ifdef BSMI_FLOOD_STATS
        if (popping) FW_STAT(5, 1);
#endif
        c = p;
      }
      hset(c, ik, ix);
    };
    // seeds in raster order, age 0
    for (int i0 = 0; i0 < n; i0 += 64) {
      const int i = i0 + lane;
      const int li = i < n ? lab[i] : 0;
      unsigned long long seeds = __ballot(li != 0);
      while (seeds) {
        const int k = __ffsll(seeds) - 1;
        seeds &= seeds - 1;
        const int j = i0 + k;
        push((MAXD2 - (uint64_t)(uint32_t)uni(d2[j])) << 32, (uint32_t)j);
      }
    }
    uint32_t age = 0;
    const int k4 = lane & 3;  // lanes 4-63 repeat lanes 0-3's neighbour fetches (same addresses: no extra lines)
    const int dq = k4 == 0 ? -W : (k4 == 1 ? -1 : (k4 == 2 ? 1 : W));
    // y = idx / W by a multiply: m = ceil(2^36 / W) = (2^36 + e) / W with 0 <= e < W, so idx * m / 2^36 = idx / W + idx * e / (W 2^36),
    // and the error term is < 1 / W -- it cannot carry past the next integer -- whenever idx * e < 2^36, which holds for
    // idx < 2^24 (the handle's H * W <= 4096^2) and W <= 4096 (the launcher refuses wider rows).  (The 32-bit reciprocal of
    // ws_flood_kernel is exact only for idx < 2^20.)
    const uint64_t mW = (((uint64_t)1 << 36) + (uint64_t)W - 1) / (uint64_t)W;
    // window of a sift-down: lane l < 62 holds the node at depth k = log2(l + 2) under the window root, position l + 2 - 2^k
    const int wl_k = 31 - __builtin_clz((uint32_t)lane + 2);
    const int wl_j = lane + 2 - (1 << wl_k);
#ifdef BSMI_FLOOD_STATS
    popping = true;
    t0 = __builtin_amdgcn_s_memrealtime();
#endif
    while (items > 0) {
      FW_STAT(0, 1);
      const uint64_t ek = hk[0];
      const uint32_t ex = hx[0];
      (void)ek;
      items = uni(items - 1);
      const int idx = uni((int)ex);
      const int y = (int)(((uint64_t)(uint32_t)idx * mW) >> 36), x = idx - y * W;
      // neighbour order [-W, -1, +1, +W]: lane k looks at neighbour k & 3
      const bool okk = k4 == 0 ? y > 0 : (k4 == 1 ? x > 0 : (k4 == 2 ? x < W - 1 : y < H - 1));
      const int qk = okk ? idx + dq : idx;
      const int lme = lab[idx], mk = mask[qk], lk = lab[qk], dk = d2[qk];
      if (items > 0) {
        // sift the last element down from the root (skimage heappop order): the smaller child, the left one on a tie
        const Ent le = hget(items);
        FW_STAT(7, items >= LH ? 1 : 0);
        const uint64_t lastk = le.k;
        const uint32_t lastx = le.x;
        int i = 0;
        bool placed = false;
        while (true) {  // LDS levels
          const int c1 = 2 * i + 1, c2 = c1 + 1;
          if (c1 >= items) { placed = true; break; }
          if (c1 >= LH) break;  // i is on the bottom LDS level: the children are spilled
          const uint64_t v1 = hk[c1], v2 = hk[c2];  // (c2 < LH; entry c2 = items is read and not looked at)
          int sm = i;
          uint64_t smv = lastk;
          if (smaller(v1, smv)) { sm = c1; smv = v1; }
          if (c2 < items && smaller(v2, smv)) { sm = c2; smv = v2; }
          if (sm == i) { placed = true; break; }
          hk[i] = smv;
          hx[i] = hx[sm];
          FW_STAT(1, 1);
          i = sm;
        }
        while (!placed) {  // spilled levels, five at a time
          uint64_t wk = 0;
          uint32_t wx = 0;
          {
            const uint32_t q = ((uint32_t)(i + 1) << wl_k) - 1 + (uint32_t)wl_j;  // < 2^30: i < 2^24, wl_k <= 5
            if (lane < 62 && q < (uint32_t)items) { wk = gk[q - LH]; wx = gx[q - LH]; }
          }
          FW_STAT(2, 1);
          int wj = 0;  // position of i in its level of the window (the root: level 0, position 0)
          int kk = 0;
          for (; kk < 5; ++kk) {
            const int c1 = 2 * i + 1, c2 = c1 + 1;
            if (c1 >= items) { placed = true; break; }
            const int l1 = (2 << kk) - 2 + 2 * wj;  // lane of c1 (c2: l1 + 1)
            const uint64_t v1 = rl64(wk, l1), v2 = rl64(wk, l1 + 1);
            int sm = i, sl = 0;
            uint64_t smv = lastk;
            if (smaller(v1, smv)) { sm = c1; smv = v1; sl = l1; }
            if (c2 < items && smaller(v2, smv)) { sm = c2; smv = v2; sl = l1 + 1; }
            if (sm == i) { placed = true; break; }
            hset(i, smv, (uint32_t)__builtin_amdgcn_readlane((int)wx, sl));
            FW_STAT(3, 1);
            wj = 2 * wj + (sm == c2 ? 1 : 0);
            i = uni(sm);
          }
        }
        hset(i, lastk, lastx);
      }
      const int l = uni(lme);
      const bool cand = okk && mk && lk == 0;
      // the neighbours to take, in the order [-W, -1, +1, +W]
      for (uint32_t m = (uint32_t)__ballot(cand) & 0xfu; m; m &= m - 1) {
        const int k = __ffs((int)m) - 1;
        const int q = __builtin_amdgcn_readlane(qk, k);
        const uint64_t dd = (uint64_t)(uint32_t)__builtin_amdgcn_readlane(dk, k);
        ++age;
        lab[q] = l;
        push(((MAXD2 - dd) << 32) | age, (uint32_t)q);
      }
    }
#ifdef BSMI_FLOOD_STATS
    st[9] = __builtin_amdgcn_s_memrealtime() - t0;
    st[10] = 1;
    if (lane == 0) {
      for (int k = 0; k < 11; ++k)
        if (k == 8) atomicMax(&g_flood_stats[k], (unsigned long long)st[k]);
        else atomicAdd(&g_flood_stats[k], (unsigned long long)st[k]);
    }
#endif
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  const uint64_t off = s.offs[z];
  uint64_t* out = frags + (size_t)z * n;
  for (int i = lane; i < n; i += 64) {
    const int l = lab[i];
    out[i] = l ? (uint64_t)l + off : 0ull;
  }
}

// return_seeds of the xy mode: slice-local seed labels + the slice's id offset (ws.py:24, 82-90)
__global__ void ws_seeds_out_kernel(int D, size_t n, WsScratch s, uint64_t* __restrict__ seeds) {
  const size_t total = (size_t)D * n;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
    const int l = s.seedlab[p];
    seeds[p] = l ? (uint64_t)l + s.offs[p / n] : 0ull;
  }
}

}  // namespace bsmi

using namespace bsmi;

static size_t ws_seeds_lds_bytes(int H, int W) {
  const size_t hw16 = ((size_t)H * W + 15) & ~(size_t)15;
  return (((size_t)H * (W + 2) * 2 + 15) & ~(size_t)15) + (((size_t)H * W * 2 + 15) & ~(size_t)15) + 2 * hw16;
}
static bool ws_seeds_use_lds(int H, int W) {
  return ws_seeds_lds_bytes(H, W) <= 158 * 1024 && (size_t)H * H + (size_t)W * W < 65535 && (H + 1) * (H + 1) + W * W < 65535;
}
static bool flood_compact_ok() {
  static const bool ok = [] { const char* e = getenv("BSMI_FLOOD_COMPACT"); return !(e && e[0] == '0'); }();
  return ok;
}

namespace bsmi {

size_t batch_ws_lds_bytes(int H, int W) {
  return ws_seeds_use_lds(H, W) && flood_compact_ok() && (size_t)H * W < ((size_t)1 << 20) ? ws_seeds_lds_bytes(H, W) : 0;
}

// Seeds of every block, then the offsets, then the floods: a seed workgroup needs a whole CU's LDS, and a CU that holds a flood
// workgroup has none to give -- in one stream, every block's seeds are through before the first flood starts.
int batch_ws_launch(const BatchBlock* tab, int N, int D, int H, int W, int msd, hipStream_t s) {
  const size_t lds = batch_ws_lds_bytes(H, W);
  if (!lds) BSMI_FAIL(BSMI_ERR_INVALID, "slices of %d x %d are off the LDS / compact path: not served in batches", H, W);
  static DeviceOnce once;
  const int rc_once = once.run([&]() -> int {
    BSMI_HIP(hipFuncSetAttribute((const void*)ws_seeds_batch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 158 * 1024));
    return BSMI_OK;
  });
  if (rc_once) return rc_once;
  hipLaunchKernelGGL(ws_seeds_batch_kernel, dim3(D, N), dim3(WS_T), lds, s, tab, D, H, W, msd, 1);
  hipLaunchKernelGGL(ws_offsets_batch_kernel, dim3(1, N), dim3(64), 0, s, tab, D);
  hipLaunchKernelGGL(ws_flood_batch_kernel, dim3((D + FLOOD_WAVES - 1) / FLOOD_WAVES, N), dim3(64 * FLOOD_WAVES), 0, s, tab, D, H, W);
  return BSMI_OK;
}

}  // namespace bsmi

static int fragments_xy(bsmi_seg* h, const uint8_t* affs_dev, int D, int H, int W, int min_seed_distance, uint64_t* frags_dev,
                        uint64_t* max_id_dev, uint64_t* seeds_dev, hipStream_t s) {
  // Slices of 2^20 voxels and more take ws_flood_wide_kernel, whose row index is exact for W <= 4096 and whose keys hold
  // d2 < 2^25, i.e. H, W <= 4096.  check_seg_shape bounds a call's slice by the handle's H * W only, so a call may lay that
  // area out as a longer row (e.g. 2796 x 6000 on a 4096 x 4096 handle): refused here, before anything runs.  (Such calls
  // were refused before the wide flood existed: no handle took slices this large.)
  if ((size_t)H * W >= ((size_t)1 << 20) && (H > 4096 || W > 4096))
    BSMI_FAIL(BSMI_ERR_INVALID, "slices of 2^20 voxels or more must have H, W <= 4096 (got %d x %d)", H, W);
  WsScratch wsx = h->ws;
  bool compact = false;  // the flood's per-voxel state as one 32-bit record (set with the seeds kernel's LDS path below)
  wsx.seedlab = nullptr;
  if (seeds_dev) {
    if (!h->seedlab) {  // allocated on first use
      void* q = nullptr;
      BSMI_HIP(hipMalloc(&q, h->max_vox * sizeof(int32_t)));
      h->allocs.push_back(q);
      h->seedlab = (int32_t*)q;
    }
    wsx.seedlab = h->seedlab;
  }
  {
    // squared distances must fit the uint16 intermediates of the LDS path: H^2 + W^2 < 65535
    // sg u16 [H][W+2] | sd2 u16 [H*W] | smask u8 [H*W] | sflag u8 [H*W], each 16-byte aligned (ws_seeds_kernel)
    const size_t lds = ws_seeds_lds_bytes(H, W);
    const bool use_lds = ws_seeds_use_lds(H, W);
    // (then also H * W < 32768: a slice's marker labels and voxel indices fit the compact record's 16 bits)
    compact = use_lds && flood_compact_ok();
    if (use_lds) {
      static DeviceOnce once;
      const int rc_once = once.run([&]() -> int {
        BSMI_HIP(hipFuncSetAttribute((const void*)ws_seeds_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 158 * 1024));
        return BSMI_OK;
      });
      if (rc_once) return rc_once;
      hipLaunchKernelGGL(ws_seeds_kernel<true>, dim3(D), dim3(WS_T), lds, s, affs_dev, D, H, W, min_seed_distance, wsx, compact ? 1 : 0);
    } else {
      hipLaunchKernelGGL(ws_seeds_kernel<false>, dim3(D), dim3(WS_T), 0, s, affs_dev, D, H, W, min_seed_distance, wsx, 0);
    }
  }
  hipLaunchKernelGGL(ws_offsets_kernel, dim3(1), dim3(64), 0, s, D, h->ws, max_id_dev);
  if (seeds_dev)
    hipLaunchKernelGGL(ws_seeds_out_kernel, dim3((unsigned)std::min<size_t>(((size_t)D * H * W + 255) / 256, 4096)), dim3(256), 0, s, D,
                       (size_t)H * W, wsx, seeds_dev);
  if ((size_t)H * W >= ((size_t)1 << 20)) {
    // beyond the packed entry's 20-bit voxel and age fields: one slice per workgroup, the heap's top levels in LDS
    if (!h->flood_spill_idx) BSMI_FAIL(BSMI_ERR_STATE, "wide flood without its spill");
    hipLaunchKernelGGL(ws_flood_wide_kernel, dim3(D), dim3(64), 0, s, D, H, W, h->ws, h->flood_spill, h->flood_spill_idx,
                       h->flood_spill_stride, frags_dev);
  } else if (compact)
    hipLaunchKernelGGL(ws_flood_kernel<true>, dim3((D + FLOOD_WAVES - 1) / FLOOD_WAVES), dim3(64 * FLOOD_WAVES), 0, s, D, H, W, h->ws, h->flood_spill,
                       h->flood_spill_stride, frags_dev, h->status_dev);
  else
    hipLaunchKernelGGL(ws_flood_kernel<false>, dim3((D + FLOOD_WAVES - 1) / FLOOD_WAVES), dim3(64 * FLOOD_WAVES), 0, s, D, H, W, h->ws, h->flood_spill,
                       h->flood_spill_stride, frags_dev, h->status_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

extern "C" {

int bsmi_ws_fragments_u8(bsmi_seg* h, const uint8_t* affs_dev, const int64_t shape[3], int fragments_in_xy,
                         int min_seed_distance, uint64_t* frags_dev, uint64_t* max_id_dev, void* stream) {
  return bsmi_ws_fragments_seeds_u8(h, affs_dev, shape, fragments_in_xy, min_seed_distance, frags_dev, max_id_dev, nullptr, stream);
}

int bsmi_ws_fragments_seeds_u8(bsmi_seg* h, const uint8_t* affs_dev, const int64_t shape[3], int fragments_in_xy,
                               int min_seed_distance, uint64_t* frags_dev, uint64_t* max_id_dev, uint64_t* seeds_dev, void* stream) {
  int rc = check_seg_shape(h, shape);
  if (rc) return rc;
  if (!affs_dev || !frags_dev || !max_id_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (min_seed_distance < 1 || min_seed_distance > 64) BSMI_FAIL(BSMI_ERR_INVALID, "min_seed_distance out of range");
  BSMI_HIP(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  const int D = (int)shape[0], H = (int)shape[1], W = (int)shape[2];
  if (!fragments_in_xy) return fragments_3d(h, affs_dev, D, H, W, min_seed_distance, frags_dev, max_id_dev, seeds_dev, s);
  return fragments_xy(h, affs_dev, D, H, W, min_seed_distance, frags_dev, max_id_dev, seeds_dev, s);
}

}  // extern "C"
